"""csrc/batchnorm.hip and the 2-D pooling kernels of csrc/elementwise.hip, stage by stage through their own bindings,
against the references of tests/bn_pool_edge_cases.py.

* sums (bn_stats, bn_bwd_reduce, the second-BN sums of bn_bwd_apply, maxpool_bwd_bnred) on integer data: equal to the
  fp64 oracle over the *expected* masks / gradients, never another launch of a kernel;
* bn_apply / bn_bwd_apply / avg pooling element by element under the derived bound ``apply_bound``;
* bn_finalize / the backward coefficients in fp32 ulps; end to end against fp64 autograd with the fp32 CPU error as
  the yardstick; measured values and the tolerances taken from them: profiles/bn_pool_edge_errors.txt;
* max pooling bit for bit against a pure-torch oracle (values, tap bytes, gradients, -inf windows, NaN).

Outputs of the streaming passes are views of larger canary-filled buffers: a row written past the end is seen.
"""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import bn_pool_edge_cases as bp  # noqa: E402

pytestmark = pytest.mark.gpu

BF, CL = torch.bfloat16, torch.channels_last
DEV = "cuda"
EPS, MOM = 1e-3, 0.1
CANARY = -77.0

# fp32 ulps allowed on bn_finalize / bn_bwd_coeff outputs: twice the largest distance measured on an MI355X, rounded up
# (profiles/bn_pool_edge_errors.txt "ulp distances"), and never more than 16
ULP_TOL = {"save_mean": 1, "save_invstd": 4, "scale": 4, "shift": 6, "running_mean": 6, "running_var": 5,
           "A": 1, "B": 6, "D": 9, "dgamma": 4, "dbeta": 3}
assert max(ULP_TOL.values()) <= 16
# end to end: allowed ratio to the yardstick = 1.5 x the largest measured (same profile, "end to end"), capped at 4.
# dres measured 0: it is the masked dz, bit for bit. The yardstick of the fp32-kept tensors is dominated by the bf16
# rounding of the fp64 result, hence their small ratios; what holds them tightly is fp32_sum_bounds (ratio <= 1)
E2E_TOL = {"y": 1.5, "dx": 1.5, "dres": 0.0, "dgamma": 1.2e-3, "dbeta": 1.3e-4, "running_mean": 1.6e-4,
           "running_var": 6.5e-5}
assert max(E2E_TOL.values()) <= 4.0


def _n():
    from bigdl_amd.ops import native

    C_ = native.get()
    assert C_.STAT_SLOTS == bp.STAT_SLOTS
    return C_


def _slots(C):
    return torch.zeros(bp.STAT_SLOTS * 2 * C, dtype=torch.float32, device=DEV)


def _slot_sums(buf, C):
    s = buf.view(-1, 2, C).double().sum(0)
    return s[0], s[1]


def _guarded(P, C, dtype=BF, per_row=None):
    """(view of P rows, whole buffer) with two canary rows after the view."""
    w = C if per_row is None else per_row
    full = torch.full(((P + 2) * w,), CANARY if dtype != torch.uint8 else 0xA5, dtype=dtype, device=DEV)
    return full[:P * w].view(P, w) if per_row is None else full[:P * w], full


def _canary_ok(full, P, w):
    tail = full[P * w:]
    return bool((tail == (0xA5 if full.dtype == torch.uint8 else CANARY)).all())


def _eq(a, b):
    return torch.equal(a.double().cpu(), b.double().cpu())


def _bits(a, b):
    """Bit equality of two bf16 tensors (signed zeros and NaN payloads included)."""
    return torch.equal(a.contiguous().view(torch.int16).cpu(), b.contiguous().view(torch.int16).cpu())


# ================================================================== exact sums
def _stats_case(P, C):
    x = bp.stats_inputs(P, C)
    buf = _slots(C)
    _n().bn_stats(x.to(DEV), buf, P, C)
    s1, s2 = _slot_sums(buf, C)
    e1, e2 = bp.stats_oracle(x)
    assert _eq(s1, e1) and _eq(s2, e2), (P, C)


def _reduce_case(P, C, kind):
    x, dz, mean = bp.int_rows(P, C, 1), bp.int_rows(P, C, 2, bp.DMAX), bp.half_means(C, 1)
    z, zm, aff, m = bp.mask_inputs(kind, P, C, x)
    buf = _slots(C)
    d = lambda t: None if t is None else t.to(DEV)      # noqa: E731
    _n().bn_bwd_reduce(dz.to(DEV), d(z), x.to(DEV), mean.to(DEV), buf, P, C, d(aff), d(zm))
    s1, s2 = _slot_sums(buf, C)
    e1, e2 = bp.bwd_reduce_oracle(dz, x, mean, m)
    assert _eq(s1, e1) and _eq(s2, e2), (P, C, kind)


def _bwd_apply_case(P, C, kind):
    """Integer dz / x and coefficients that are exact in fp32: every intermediate of dx = A dy + B x + D is an fp32
    number, so dx is the bf16 rounding of the exact value, bit for bit; dres is the masked dz; the second-BN sums are
    the oracle's over that expected dres, with and without dres / dx being written."""
    C_ = _n()
    x, dz, x2 = bp.int_rows(P, C, 1), bp.int_rows(P, C, 2, bp.DMAX), bp.int_rows(P, C, 3)
    mean2 = bp.half_means(C, 2)
    z, zm, aff, m = bp.mask_inputs(kind, P, C, x)
    invstd, gamma, mean, red = bp.exact_coef_inputs(C, P, 1)
    co = bp.coeff_ref(red, 1, mean, invstd, gamma, P, True)
    want_dx, _, dy = bp.bwd_apply_ref(dz, x, m, co)
    want_dx, want_dres = want_dx.float().to(BF), dy.to(BF)
    e1, e2 = bp.bwd_reduce_oracle(want_dres, x2, mean2, torch.ones(P, C, dtype=torch.bool))
    d = lambda t: None if t is None else t.to(DEV)      # noqa: E731
    args = (d(dz), d(z), d(x), d(mean), d(invstd), d(gamma), d(red), 1)
    for sec, need_dres, need_dx in ((False, True, True), (True, True, True), (True, False, True), (True, False, False)):
        coef = torch.empty(3 * C, dtype=torch.float32, device=DEV)
        dg, db = torch.full((C,), 3.0, device=DEV), torch.full((C,), -2.0, device=DEV)
        dx, dxf = _guarded(P, C) if need_dx else (None, None)
        dres, drf = _guarded(P, C) if need_dres else (None, None)
        red2 = _slots(C) if sec else None
        kw = dict(x2=d(x2), mean2=d(mean2), red2=red2) if sec else {}
        C_.bn_bwd_apply(*args, coef, dx, dres, dg, db, P, C, d(aff), d(zm), **kw)
        tag = (P, C, kind, sec, need_dres, need_dx)
        assert _eq(coef, torch.cat([co["A"], co["B"], co["D"]])), tag
        assert _eq(dg, 3.0 + co["dgamma"]) and _eq(db, -2.0 + co["dbeta"]), tag
        if need_dx:
            assert _bits(dx, want_dx) and _canary_ok(dxf, P, C), tag
        if need_dres:
            assert _bits(dres, want_dres) and _canary_ok(drf, P, C), tag
        if sec:
            s1, s2 = _slot_sums(red2, C)
            assert _eq(s1, e1) and _eq(s2, e2), tag


def _apply_exact_case(P, C):
    """Integer x / res, power-of-two scale, half-integer shift: y is exact, so bf16 bit equality; the sign bytes equal
    y > 0. Plain, residual + ReLU, and the shortcut affine (RA) on load."""
    C_ = _n()
    g = bp._gen(P, C, 41)
    x, res = bp.int_rows(P, C, 1), bp.int_rows(P, C, 4)
    scale = 2.0 ** torch.randint(-1, 2, (C,), generator=g).float() * (1 - 2 * torch.randint(0, 2, (C,), generator=g)).float()
    shift, rsh = bp.half_means(C, 3), bp.half_means(C, 4)
    rsc = 2.0 ** torch.randint(-1, 2, (C,), generator=g).float()
    for mode in ("plain", "res+relu", "ra+relu"):
        want = x.double() * scale.double() + shift.double()
        if mode != "plain":
            want = want + (res.double() if mode == "res+relu" else res.double() * rsc.double() + rsh.double())
            want = want.clamp_min(0)
        y, yf = _guarded(P, C)
        zm, zf = _guarded(P, C, torch.uint8, C // 8)
        ra = (rsc.to(DEV), rsh.to(DEV)) if mode == "ra+relu" else (None, None)
        C_.bn_apply(x.to(DEV), scale.to(DEV), shift.to(DEV), None if mode == "plain" else res.to(DEV), y, P, C,
                    mode != "plain", zm, *ra)
        assert _bits(y, want.to(BF)) and _canary_ok(yf, P, C), (P, C, mode)
        assert torch.equal(zm.cpu(), bp.pack_mask(want > 0)) and _canary_ok(zf, P, C // 8), (P, C, mode)


@pytest.mark.parametrize("C", bp.BN_CHANNELS)
def test_bn_stats_sums_are_exact(C):
    for P in bp.row_counts(C):
        _stats_case(P, C)


@pytest.mark.parametrize("kind", bp.MASKS)
@pytest.mark.parametrize("C", bp.BN_CHANNELS)
def test_bn_bwd_reduce_sums_are_exact_under_every_mask(C, kind):
    for P in bp.row_counts(C):
        _reduce_case(P, C, kind)


@pytest.mark.parametrize("kind", bp.MASKS)
@pytest.mark.parametrize("C", bp.BN_CHANNELS)
def test_bn_bwd_apply_is_bit_exact_on_integer_data(C, kind):
    for P in bp.row_counts(C):
        _bwd_apply_case(P, C, kind)


@pytest.mark.parametrize("C", bp.BN_CHANNELS)
def test_bn_apply_is_bit_exact_on_integer_data(C):
    for P in bp.row_counts(C):
        _apply_exact_case(P, C)


def _exact_subset():
    """What a child interpreter runs under BIGDL_BN_UNROLL = 1, 2, 8: the integer-exact checks on the small shapes."""
    for C in (8, 24, 88, 2056):
        for P in bp.row_counts(C):
            _stats_case(P, C)
            _apply_exact_case(P, C)
            for kind in ("none", "zm", "aff"):
                _reduce_case(P, C, kind)
                _bwd_apply_case(P, C, kind)


@pytest.mark.parametrize("U", [1, 2, 8])
def test_unroll_variants_in_a_fresh_interpreter(U):
    """BIGDL_BN_UNROLL is read once per process."""
    env = dict(os.environ, BIGDL_BN_UNROLL=str(U))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--exact-subset"], env=env, cwd=ROOT, timeout=240,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and f"exact subset ok U={U}" in r.stdout, r.stdout[-2000:]


# ------------------------------------------------------------------ block caps (the workload's branches)
def _dev_ints(P, C, lim, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(-lim, lim + 1, (P, C), generator=g, device=DEV, dtype=torch.int8).to(BF)


def test_reduce_past_the_2048_block_cap():
    C, P = bp.REDUCE_CAP
    assert bp.reduce_geometry(P, C)[2]
    C_ = _n()
    x, dz = _dev_ints(P, C, bp.XMAX, 1), _dev_ints(P, C, bp.DMAX, 2)
    x[P - 1] = 4.0
    mean, aff = bp.half_means(C, 1).to(DEV), bp.aff_exact(C, 3).to(DEV)
    buf = _slots(C)
    C_.bn_stats(x, buf, P, C)
    s1, s2 = _slot_sums(buf, C)
    e1, e2 = bp.stats_oracle(x)
    assert _eq(s1, e1) and _eq(s2, e2)
    zm = ((torch.arange(P * C // 8, device=DEV) * 37 + 11) % 256).to(torch.uint8)
    for kw, m in ((dict(aff=aff), bp.aff_pre(x, aff) > 0), (dict(zm=zm), bp.unpack_mask(zm, P, C))):
        buf = _slots(C)
        C_.bn_bwd_reduce(dz, None, x, mean, buf, P, C, **kw)
        s1, s2 = _slot_sums(buf, C)
        e1, e2 = bp.bwd_reduce_oracle(dz, x, mean, m)
        assert _eq(s1, e1) and _eq(s2, e2), list(kw)


def test_apply_passes_past_the_8192_block_cap():
    """bx > 8192 / gy with two channel-group chunks: rows per block are re-cut and the last blocks start past P."""
    C, P = bp.APPLY_CAP
    assert bp.stationary_geometry(P, C)[3]
    C_ = _n()
    g = bp._gen(P, C, 43)
    x, dz, x2, res = (_dev_ints(P, C, 4, s) for s in (1, 2, 3, 4))
    scale = (2.0 ** torch.randint(-1, 2, (C,), generator=g).float()).to(DEV)
    shift, mean2 = bp.half_means(C, 3).to(DEV), bp.half_means(C, 2).to(DEV)
    want = (x.double() * scale.double() + shift.double() + res.double()).clamp_min(0)
    y, yf = _guarded(P, C)
    zm, zf = _guarded(P, C, torch.uint8, C // 8)
    C_.bn_apply(x, scale, shift, res, y, P, C, True, zm)
    assert _bits(y, want.to(BF)) and _canary_ok(yf, P, C)
    m = want > 0
    assert torch.equal(zm, bp.pack_mask(m)) and _canary_ok(zf, P, C // 8)
    del want
    invstd, gamma, mean, red = bp.exact_coef_inputs(C, P, 1)
    co = {k: v.to(DEV) for k, v in bp.coeff_ref(red, 1, mean, invstd, gamma, P, True).items()}
    want_dx, _, dy = bp.bwd_apply_ref(dz, x, m, co)
    want_dx, want_dres = want_dx.float().to(BF), dy.to(BF)
    del dy
    coef = torch.empty(3 * C, dtype=torch.float32, device=DEV)
    dx, dxf = _guarded(P, C)
    dres, drf = _guarded(P, C)
    red2 = _slots(C)
    C_.bn_bwd_apply(dz, None, x, mean.to(DEV), invstd.to(DEV), gamma.to(DEV), red.to(DEV), 1, coef, dx, dres, None,
                    None, P, C, None, zm, x2=x2, mean2=mean2, red2=red2)
    assert _bits(dx, want_dx) and _canary_ok(dxf, P, C)
    assert _bits(dres, want_dres) and _canary_ok(drf, P, C)
    s1, s2 = _slot_sums(red2, C)
    e1, e2 = bp.bwd_reduce_oracle(want_dres, x2, mean2, torch.ones(1, 1, dtype=torch.bool, device=DEV))
    assert _eq(s1, e1) and _eq(s2, e2)


def test_deterministic_reduce_at_its_slot_cap():
    """Deterministic mode caps the reduction at 2 * STAT_SLOTS blocks: still exact, and the slot buffer itself is
    bit-equal over two runs (at most two addends per word)."""
    from bigdl_amd.ops import native

    C, P = bp.DET_CAP
    assert bp.reduce_geometry(P, C, det=True)[2]
    C_ = _n()
    x, dz, mean = bp.stats_inputs(P, C).to(DEV), bp.int_rows(P, C, 2).to(DEV), bp.half_means(C, 1).to(DEV)
    was = native.deterministic()
    native.set_deterministic(True)
    try:
        bufs = []
        for _ in range(2):
            a, b = _slots(C), _slots(C)
            C_.bn_stats(x, a, P, C)
            C_.bn_bwd_reduce(dz, None, x, mean, b, P, C)
            bufs.append((a, b))
    finally:
        native.set_deterministic(was)
    assert torch.equal(bufs[0][0], bufs[1][0]) and torch.equal(bufs[0][1], bufs[1][1])
    # at most 2 * STAT_SLOTS blocks wrote: every slot holds something, none more than two blocks' rows of |x| <= 4
    rpb = bp.reduce_geometry(P, C, det=True)[1]
    assert bufs[0][0].view(-1, 2, C)[:, 0].abs().max().item() <= 2 * rpb * bp.XMAX
    s1, s2 = _slot_sums(bufs[0][0], C)
    e1, e2 = bp.stats_oracle(x)
    assert _eq(s1, e1) and _eq(s2, e2)
    s1, s2 = _slot_sums(bufs[0][1], C)
    e1, e2 = bp.bwd_reduce_oracle(dz, x, mean, torch.ones(1, 1, dtype=torch.bool, device=DEV))
    assert _eq(s1, e1) and _eq(s2, e2)


# ================================================================== finalize / coefficients in ulps
def _ulp_check(tag, got, ref, names, worst):
    bad = []
    for n in names:
        at = ref.get(n + "_terms") if n in ("shift", "running_mean", "running_var", "D") else None
        u = bp.ulps(got[n], ref[n], at)
        worst[n] = max(worst.get(n, 0.0), u)
        print(f"EDGE_ULP {tag} {n} {u:.2f}")
        if not u <= ULP_TOL[n]:
            bad.append((n, u))
    assert not bad, (tag, bad)


@pytest.mark.parametrize("fill", ["all", "high", "one"])
@pytest.mark.parametrize("C", [8, 24, 64, 2056])
def test_finalize_and_coefficients_from_synthetic_slots(C, fill):
    C_ = _n()
    nslots = 1 if fill == "one" else bp.STAT_SLOTS
    worst = {}
    for P, affine in ((1000, True), (1000, False), (2, True), (1, True)):
        stats = bp.slot_buffer(C, nslots, fill, 1, P=P)
        g = bp._gen(C, P, 47)
        gamma = torch.randn(C, generator=g) if affine else None
        beta = torch.randn(C, generator=g) if affine else None
        rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
        ref = bp.finalize_ref(stats, nslots, gamma, beta, rm0, rv0, P, EPS, MOM, True)
        d = lambda t: None if t is None else t.to(DEV)      # noqa: E731
        out = {n: torch.full((C + 8,), CANARY, device=DEV) for n in ("save_mean", "save_invstd", "scale", "shift")}
        rm, rv = rm0.to(DEV), rv0.to(DEV)
        C_.bn_finalize(stats.to(DEV), nslots, d(gamma), d(beta), rm, rv, out["save_mean"][:C], out["save_invstd"][:C],
                       out["scale"][:C], out["shift"][:C], P, C, EPS, MOM, True)
        assert all(bool((v[C:] == CANARY).all()) for v in out.values())          # nothing written past channel C
        got = {n: v[:C] for n, v in out.items()}
        got.update(running_mean=rm, running_var=rv)
        _ulp_check(f"finalize C={C} {fill} P={P} affine={int(affine)}", got, ref,
                   ("save_mean", "save_invstd", "scale", "shift", "running_mean", "running_var"), worst)
        # backward coefficients from a synthetic reduction, dgamma / dbeta added onto non-zero values
        red = bp.slot_buffer(C, nslots, fill, 2, mean=1.0, P=P)
        mean, invstd = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.3
        cref = bp.coeff_ref(red, nslots, mean, invstd, gamma, P, True)
        coef = torch.full((3 * C + 8,), CANARY, device=DEV)
        dg0, db0 = torch.randn(C, generator=g), torch.randn(C, generator=g)
        dg, db = dg0.to(DEV), db0.to(DEV)
        one = torch.zeros(1, C, dtype=BF, device=DEV)
        C_.bn_bwd_apply(one, None, one, mean.to(DEV), invstd.to(DEV), d(gamma), red.to(DEV), nslots, coef[:3 * C],
                        None, None, dg, db, P, C)
        assert bool((coef[3 * C:] == CANARY).all())
        gotc = {"A": coef[:C], "B": coef[C:2 * C], "D": coef[2 * C:3 * C], "dgamma": dg.cpu() - dg0, "dbeta": db.cpu() - db0}
        # the increments are read back after an fp32 add onto the start values: one more rounding at their size
        for n in ("dgamma", "dbeta"):
            at = cref[n].abs().maximum(dg0.double().abs() if n == "dgamma" else db0.double().abs())
            u = bp.ulps(gotc[n], cref[n], at)
            worst[n] = max(worst.get(n, 0.0), u)
            print(f"EDGE_ULP coeff C={C} {fill} P={P} {n} {u:.2f}")
            assert u <= ULP_TOL[n], (n, u)
        _ulp_check(f"coeff C={C} {fill} P={P} affine={int(affine)}", gotc, cref, ("A", "B", "D"), worst)
    print("EDGE_ULP_WORST", C, fill, {k: round(v, 2) for k, v in worst.items()})


def test_finalize_eval_mode_clamp_and_backward_without_statistics():
    C_ = _n()
    C = 24
    g = bp._gen(C, 53)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    worst = {}
    # eval: mean / variance are the running ones, which stay untouched; save_mean / save_invstd optional
    for with_save in (True, False):
        ref = bp.finalize_ref(None, 0, gamma, beta, rm0, rv0, 7, EPS, MOM, False)
        rm, rv = rm0.to(DEV), rv0.to(DEV)
        sm, si, sc, sh = (torch.full((C,), CANARY, device=DEV) for _ in range(4))
        C_.bn_finalize(sc, 0, gamma.to(DEV), beta.to(DEV), rm, rv, sm if with_save else None,
                       si if with_save else None, sc, sh, 7, C, EPS, MOM, False)
        assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0)
        names = ("scale", "shift") + (("save_mean", "save_invstd") if with_save else ())
        _ulp_check(f"finalize eval save={int(with_save)}", {"scale": sc, "shift": sh, "save_mean": sm, "save_invstd": si},
                   ref, names, worst)
    # a slot pair whose s2 / P - mean^2 is slightly negative: the clamp gives invstd = rsqrt(eps)
    P = 3
    stats = torch.zeros(1, 2, C)
    stats[0, 0], stats[0, 1] = 3.0, 2.9999998
    ref = bp.finalize_ref(stats, 1, None, None, None, None, P, EPS, MOM, True)
    assert (ref["var_raw"] < 0).all()
    sm, si, sc, sh = (torch.empty(C, device=DEV) for _ in range(4))
    C_.bn_finalize(stats.to(DEV), 1, None, None, None, None, sm, si, sc, sh, P, C, EPS, MOM, True)
    _ulp_check("finalize negative-variance", {"save_mean": sm, "save_invstd": si, "scale": sc, "shift": sh}, ref,
               ("save_mean", "save_invstd", "scale", "shift"), worst)
    # backward with training = 0 (no reduction): A = gamma invstd only, B = D = 0, dgamma / dbeta untouched; dx = A dz
    Pn = 67
    dz, x = bp.gauss_rows(Pn, C, 1), bp.gauss_rows(Pn, C, 2)
    invstd, mean = torch.rand(C, generator=g) + 0.3, torch.randn(C, generator=g)
    cref = bp.coeff_ref(None, 0, mean, invstd, gamma, Pn, False)
    coef = torch.empty(3 * C, device=DEV)
    dg, db = torch.full((C,), 5.0, device=DEV), torch.full((C,), 6.0, device=DEV)
    dx, dxf = _guarded(Pn, C)
    C_.bn_bwd_apply(dz.to(DEV), None, x.to(DEV), mean.to(DEV), invstd.to(DEV), gamma.to(DEV), None, 0, coef, dx, None,
                    dg, db, Pn, C)
    assert bool((dg == 5.0).all()) and bool((db == 6.0).all())
    assert bool((coef[C:] == 0).all())
    _ulp_check("coeff training=0", {"A": coef[:C]}, cref, ("A",), worst)
    A32 = coef[:C].cpu().double()
    want = A32 * dz.double()
    assert ((dx.cpu().double() - want).abs() <= bp.apply_bound(want, want.abs())).all() and _canary_ok(dxf, Pn, C)


# ================================================================== element-wise bounds
@pytest.mark.parametrize("mode", bp.APPLY_MODES)
@pytest.mark.parametrize("P,C", bp.APPLY_SHAPES)
def test_bn_apply_within_the_rounding_bound(P, C, mode):
    """|y - y_exact| <= (1 + 2^-6) h(y_exact) + 4 * 2^-24 (|x scale| + |shift| + |res terms|) [+ the bf16 spacing of the
    shortcut term for RA]: derived in bn_pool_edge_cases.apply_bound. The sign bytes equal y_kernel > 0 bit for bit,
    and y_exact > 0 wherever |pre-ReLU| is not below the fp32 term."""
    C_ = _n()
    d = bp.apply_inputs(P, C, mode)
    want, pre, terms, extra, pre_m = bp.bn_apply_ref(d["x"], d["scale"], d["shift"], d["res"], d["res_scale"],
                                                     d["res_shift"], d["relu"])
    y, yf = _guarded(P, C)
    zm, zf = _guarded(P, C, torch.uint8, C // 8) if d["zm"] else (None, None)
    t = lambda k: None if d[k] is None else d[k].to(DEV)      # noqa: E731
    C_.bn_apply(t("x"), t("scale"), t("shift"), t("res"), y, P, C, d["relu"], zm, t("res_scale"), t("res_shift"))
    err = (y.cpu().double() - want).abs()
    bound = bp.apply_bound(want, terms, extra)
    print(f"EDGE_BOUND bn_apply {P}x{C} {mode} worst err/bound={(err / bound).max().item():.3f}")
    assert (err <= bound).all() and _canary_ok(yf, P, C)
    if d["zm"]:
        assert torch.equal(zm.cpu(), bp.pack_mask(y.cpu().float() > 0)) and _canary_ok(zf, P, C // 8)
        decided = pre_m.abs() >= bp.fp32_term(terms)
        assert decided.double().mean().item() > 0.999
        assert torch.equal(bp.unpack_mask(zm.cpu(), P, C)[decided], (pre_m > 0)[decided])


@pytest.mark.parametrize("kind", ["none", "z", "zm", "aff"])
@pytest.mark.parametrize("P,C", bp.APPLY_SHAPES)
def test_bn_bwd_apply_dx_within_the_rounding_bound(P, C, kind):
    """Gaussian dz / x, coefficients chosen exact (bn_pool_edge_cases.exact_coef_inputs): the same bound around
    A dy + B x + D; dres is the masked dz bit for bit."""
    C_ = _n()
    x, dz = bp.gauss_rows(P, C, 31, 0.2, 1.5), bp.gauss_rows(P, C, 33)
    z = zm = aff = None
    m = torch.ones(P, C, dtype=torch.bool)
    if kind == "z":
        z = bp.gauss_rows(P, C, 35)
        z.view(-1)[::5] = 0.0
        m = z.float() > 0
    elif kind == "zm":
        zm = ((torch.arange(P * C // 8) * 37 + 11) % 256).to(torch.uint8)
        m = bp.unpack_mask(zm, P, C)
    elif kind == "aff":
        g = bp._gen(P, C, 59)
        aff = torch.cat([torch.randn(C, generator=g), torch.randn(C, generator=g)])
        m = bp.aff_pre(x, aff) > 0
    invstd, gamma, mean, red = bp.exact_coef_inputs(C, P, 2)
    co = bp.coeff_ref(red, 1, mean, invstd, gamma, P, True)
    want, terms, dy = bp.bwd_apply_ref(dz, x, m, co)
    d = lambda t: None if t is None else t.to(DEV)      # noqa: E731
    coef = torch.empty(3 * C, device=DEV)
    dx, dxf = _guarded(P, C)
    dres, drf = _guarded(P, C)
    C_.bn_bwd_apply(d(dz), d(z), d(x), d(mean), d(invstd), d(gamma), d(red), 1, coef, dx, dres, None, None, P, C, d(aff),
                    d(zm))
    assert _eq(coef, torch.cat([co["A"], co["B"], co["D"]]))
    err, bound = (dx.cpu().double() - want).abs(), bp.apply_bound(want, terms)
    print(f"EDGE_BOUND bn_bwd_apply {P}x{C} {kind} worst err/bound={(err / bound).max().item():.3f}")
    assert (err <= bound).all() and _canary_ok(dxf, P, C)
    assert _bits(dres, dy.to(BF)) and _canary_ok(drf, P, C)


# ================================================================== end to end against fp64 autograd
def _e2e(P, C, mode, worst):
    from bigdl_amd.ops import bn

    relu, with_res = mode != "plain", mode == "res+relu+zm"
    x, dz = bp.gauss_rows(P, C, 61, 0.0, 1.0), bp.gauss_rows(P, C, 63)
    res = bp.gauss_rows(P, C, 65) if with_res else None
    g = bp._gen(P, C, 67)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    hi = bp.bn_autograd(x, gamma, beta, res, relu, dz, EPS, MOM, torch.float64)
    lo = bp.bn_autograd(x, gamma, beta, res, relu, dz, EPS, MOM, torch.float32)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    zm, zf = _guarded(P, C, torch.uint8, C // 8) if with_res else (None, None)
    out, outf = _guarded(P, C)
    xd, gd = x.to(DEV), gamma.to(DEV)
    y, sm, si, aff = bn.bn_forward_gpu(xd, gd, beta.to(DEV), rm, rv, EPS, MOM, True,
                                       res=res.to(DEV) if with_res else None, relu=relu, zm=zm, out=out)
    assert _canary_ok(outf, P, C) and (zf is None or _canary_ok(zf, P, C // 8))
    dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    dx, dres = bn.bn_backward_gpu(dz.to(DEV), None, xd, sm, si, gd, dg, db, need_dres=with_res,
                                  aff=aff if mode == "relu+aff" else None, zm=zm)
    got = {"y": y, "dx": dx, "dres": dres, "dgamma": dg, "dbeta": db, "running_mean": rm, "running_var": rv}
    bad = []
    for n, v in got.items():
        if v is None:
            continue
        yard = bp.yardstick(hi, lo, n)
        err = (v.cpu().double() - hi[n]).abs().max().item()
        ratio = err / yard if yard > 0 else float(err > 0)
        if ratio > worst.get(n, (0.0,))[0]:
            worst[n] = (ratio, f"{P}x{C} {mode}")
        if not ratio <= E2E_TOL[n]:
            bad.append((n, P, C, mode, ratio))
    # the tensors kept in fp32 are sums over P rows: the yardstick above (it contains the bf16 rounding of the
    # result) says little about them, so they are also held to the accumulation bound of the kernels' own scheme
    dy = dz.double() * (hi["y"] > 0).double() if relu else dz.double()
    for n, b in bp.fp32_sum_bounds(x, dy, gamma, P, C, EPS, MOM).items():
        r = ((got[n].cpu().double() - hi[n]).abs() / b).max().item()
        if r > worst.get(n + "/acc", (0.0,))[0]:
            worst[n + "/acc"] = (r, f"{P}x{C} {mode}")
        if not r <= 1.0:
            bad.append((n + "/acc", P, C, mode, r))
    return bad


@pytest.mark.parametrize("C", bp.BN_CHANNELS)
def test_bn_forward_backward_against_fp64_autograd(C):
    """Yardstick per tensor: max(error of fp32 CPU F.batch_norm + autograd against fp64, bf16 rounding error of the
    fp64 result); allowed ratio E2E_TOL (1.5 x the largest measured, at most 4)."""
    worst, bad = {}, []
    for P in bp.row_counts(C):
        if P < 2:
            continue                    # F.batch_norm refuses one value per channel; the stage tests run P = 1
        for mode in ("plain", "relu+aff", "res+relu+zm"):
            bad += _e2e(P, C, mode, worst)
    print("EDGE_E2E", C, {k: (float(f"{v[0]:.3g}"), v[1]) for k, v in worst.items()})
    assert not bad, bad


@pytest.mark.parametrize("mu", [8.0, 64.0])
def test_offset_data_variance_within_the_one_pass_bound(mu):
    """x = mu + randn, one channel constant at 100, one all zero. The kernels form the variance as E[x^2] - E[x]^2 from
    fp32 partial sums: |var_kernel - var| <= n 2^-23 (E[x^2] + 2 mean^2) with n the longest addition chain
    (bn_pool_edge_cases.var_bound), plus the rounding of invstd itself. The invstd and y errors this leaves are
    recorded in profiles/bn_pool_edge_errors.txt ("offset data"); the one-pass scheme is a known limit there."""
    from bigdl_amd.ops import bn

    P, C = 4097, 64
    x = bp.offset_rows(P, C, mu)
    xd = x.double()
    var = xd.var(0, unbiased=False)
    inv_ref = (var + EPS).rsqrt()
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    out, outf = _guarded(P, C)
    y, sm, si, aff = bn.bn_forward_gpu(x.to(DEV), None, None, rm, rv, EPS, MOM, True, out=out)
    assert _canary_ok(outf, P, C)
    var_k = si.cpu().double() ** -2 - EPS
    bound, n = bp.var_bound(x, P, C)
    slack = 8 * 2.0 ** -24 * (var + EPS)                   # invstd is an fp32 rsqrt (2 ulp) of var + fp32(eps), squared back
    dv = (var_k - var).abs()
    rel_inv = ((si.cpu().double() - inv_ref).abs() / inv_ref)
    yref = (xd - xd.mean(0)) * inv_ref
    yerr = (y.cpu().double() - yref).abs()
    yround = (yref.to(BF).double() - yref).abs().max().item()
    print(f"EDGE_OFFSET mu={mu} n={n} gauss: dvar={dv[2:].max().item():.3e} bound={bound[2:].min().item():.3e} "
          f"invstd rel={rel_inv[2:].max().item():.3e} y err={yerr[:, 2:].max().item():.3e} (bf16 rounding {yround:.3e}); "
          f"const100: dvar={dv[0].item():.3e} bound={bound[0].item():.3e} invstd rel={rel_inv[0].item():.3e} "
          f"y err={yerr[:, 0].max().item():.3e}; zero: dvar={dv[1].item():.3e} y err={yerr[:, 1].max().item():.3e}")
    assert (dv <= bound + slack).all(), (dv / (bound + slack)).max().item()
    assert dv[1].item() <= slack[1].item() and yerr[:, 1].max().item() == 0          # the all-zero channel is exact


# ================================================================== average pooling
@pytest.mark.parametrize("count_pad", [True, False])
@pytest.mark.parametrize("case", bp.AVGPOOL_CASES, ids=lambda c: c[0])
def test_avgpool_within_the_rounding_bound(case, count_pad):
    """(1 + 2^-6) h + 4 * 2^-24 sum |terms| per element, forward and backward, against fp64 F.avg_pool2d."""
    from bigdl_amd.ops import pool

    name, (N, C, H, W), k, s, p, ceil = case
    x = bp.gauss_rows(N * H * W, C, 71, 0.3).view(N, H, W, C).permute(0, 3, 1, 2)
    OH, OW = bp.pool_out(H, k, s, p, ceil), bp.pool_out(W, k, s, p, ceil)
    dy = bp.gauss_rows(N * OH * OW, C, 73).view(N, OH, OW, C).permute(0, 3, 1, 2)
    y_ref, dx_ref, ya, dxa = bp.avgpool_ref(x, dy, k, s, p, ceil, count_pad)
    y = pool.avgpool_fwd_gpu(x.to(DEV).contiguous(memory_format=CL), k, k, s, s, p, p, ceil, count_pad)
    assert y.shape == y_ref.shape
    dx = pool.avgpool_bwd_gpu(dy.to(DEV), (N, C, H, W), k, k, s, s, p, p, count_pad)
    ey, edx = (y.cpu().double() - y_ref).abs(), (dx.cpu().double() - dx_ref).abs()
    by, bdx = bp.apply_bound(y_ref, ya), bp.apply_bound(dx_ref, dxa)
    print(f"EDGE_BOUND avgpool {name} count_pad={int(count_pad)} y={(ey / by).max().item():.3f} dx={(edx / bdx).max().item():.3f}")
    assert (ey <= by).all() and (edx <= bdx).all()


# ================================================================== max pooling (everything exact)
PRE = torch.cat([torch.tensor([0.5, 1.0, -1.0, 1.3, 0.7, 2.0, -0.3, 1.1]).to(BF).float(),
                 torch.tensor([0.0, -1.0, 0.5, 0.2, -0.4, 1.0, 0.3, -2.0]).to(BF).float()])


def _pre_for(C):
    return torch.cat([PRE[:8].repeat(C // 8), PRE[8:].repeat(C // 8)])


def _maxpool_check(x, k, s, p, ceil, pre=None, oracle_dev="cpu", dy_lim=4):
    """x: bf16 NHWC-contiguous [N, C, H, W] on the CPU or the device. Forward values, tap bytes, backward, sums."""
    from bigdl_amd.ops import pool

    N, C, H, W = x.shape
    xo = x.to(oracle_dev)
    win = bp.pre_elements(xo, pre) if pre is not None else xo
    y_ref, idx_ref = bp.maxpool_oracle(win.float(), k, s, p, ceil)
    xg = x.to(DEV).contiguous(memory_format=CL)
    y, idx = pool.maxpool_fwd_gpu(xg, k, k, s, s, p, p, ceil, None if pre is None else pre.to(DEV))
    assert y.shape == y_ref.shape
    assert _bits(y, y_ref.to(BF)), "values"
    assert torch.equal(idx.cpu(), idx_ref.cpu()), "tap bytes"
    gen = torch.Generator(device=oracle_dev).manual_seed(5)
    dy = torch.randint(-dy_lim, dy_lim + 1, y_ref.shape, generator=gen, device=oracle_dev).to(BF)
    dx_ref = bp.maxpool_bwd_oracle(dy, idx_ref, H, W, k, s, p)
    dyg = dy.to(DEV).contiguous(memory_format=CL)
    dx = pool.maxpool_bwd_gpu(dyg, idx, (N, C, H, W), k, k, s, s, p, p)
    assert _bits(dx, dx_ref.to(BF)), "dx"                    # sums of at most 9 integers |dy| <= 4: bf16-exact
    assert _eq(dx.double().sum((0, 2, 3)), dy.double().sum((0, 2, 3))), "sum dx == sum dy"
    return dyg, idx, dx_ref


@pytest.mark.parametrize("case", bp.MAXPOOL_CASES, ids=lambda c: c[0])
def test_maxpool_matches_the_oracle_bit_for_bit(case):
    name, shape, k, s, p, ceil = case
    _maxpool_check(bp.int_image(*shape, 1), k, s, p, ceil)
    if (k, s) == (3, 2):
        _maxpool_check(bp.int_image(*shape, 2), k, s, p, ceil, pre=_pre_for(shape[1]))


def test_maxpool_past_the_8192_block_cap():
    """The grid-stride loops of the fixed forward and of the k3s2 backward make a second trip."""
    name, (N, C, H, W), k, s, p, ceil = bp.MAXPOOL_BIG
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randint(-2, 3, (N, H, W, C), generator=g, device=DEV, dtype=torch.int8).to(BF).permute(0, 3, 1, 2)
    _maxpool_check(x, k, s, p, ceil, oracle_dev=DEV)


def _bnred_check(shape, kind, oracle_dev="cpu", dy_lim=4):
    """maxpool_bwd_bnred: dx bit-equal to the oracle; red equal to the fp64 sums over the expected dx under the expected
    mask (written by the test: zm bytes, or the sign of fma(x, scale, shift))."""
    from bigdl_amd.ops import pool

    N, C, H, W = shape
    g = torch.Generator(device=oracle_dev).manual_seed(7)
    img = torch.randint(-2, 3, (N, H, W, C), generator=g, device=oracle_dev, dtype=torch.int8).to(BF).permute(0, 3, 1, 2)
    bx = torch.randint(-2, 3, (N, H, W, C), generator=g, device=oracle_dev, dtype=torch.int8).to(BF).permute(0, 3, 1, 2)
    y_ref, idx_ref = bp.maxpool_oracle(img.float(), 3, 2, 1)
    dy = torch.randint(-dy_lim, dy_lim + 1, y_ref.shape, generator=g, device=oracle_dev).to(BF)
    dx_ref = bp.maxpool_bwd_oracle(dy, idx_ref, H, W, 3, 2, 1)
    mean = bp.half_means(C, 5)
    P = N * H * W
    rows = bp.nhwc_rows
    zm = aff = None
    if kind == "zm":
        zm = ((torch.arange(P * C // 8, device=oracle_dev) * 37 + 11) % 256).to(torch.uint8)
        m = bp.unpack_mask(zm, P, C)
    else:
        aff = bp.aff_exact(C, 5)
        m = bp.aff_pre(rows(bx), aff) > 0
    e1, e2 = bp.bwd_reduce_oracle(rows(dx_ref), rows(bx), mean, m)
    idx = idx_ref.to(DEV).contiguous(memory_format=CL)
    src = (None, bx.to(DEV).contiguous(memory_format=CL), mean.to(DEV), None if aff is None else aff.to(DEV),
           zm.to(DEV) if zm is not None else False)
    dx, red = pool.maxpool_bwd_bnred_gpu(dy.to(DEV).contiguous(memory_format=CL), idx, shape, 3, 3, 2, 2, 1, 1, src)
    assert _bits(dx, dx_ref.to(BF))
    if 256 % (C // 8) != 0:
        assert red is None                              # the fused kernel must decline: a thread's group would move
        return
    assert red is not None
    s1, s2 = _slot_sums(red, C)
    assert _eq(s1, e1) and _eq(s2, e2)


@pytest.mark.parametrize("kind", ["zm", "aff"])
@pytest.mark.parametrize("shape", bp.BNRED_CASES + [(2, 24, 6, 4)], ids=str)
def test_maxpool_bwd_bnred_sums_over_the_expected_gradient(shape, kind):
    _bnred_check(shape, kind)


def test_maxpool_bwd_bnred_past_its_2048_block_cap():
    _bnred_check(bp.BNRED_BIG, "zm", oracle_dev=DEV, dy_lim=2)


@pytest.mark.parametrize("k,s,p,shape,pre", [(3, 2, 1, (1, 8, 4, 4), False), (3, 2, 1, (2, 8, 5, 7), False),
                                             (3, 1, 1, (1, 8, 4, 3), False), (5, 2, 2, (1, 8, 5, 5), False),
                                             (3, 2, 1, (1, 8, 4, 4), True)])
def test_all_minus_inf_windows_keep_a_winner_inside_the_image(k, s, p, shape, pre):
    """A window whose in-bounds values are all -inf: the winner is the first in-bounds tap, as in torch, so the
    backward still delivers the gradient (sum dx == sum dy). Whole image -inf, and a -inf corner block only."""
    for whole in (True, False):
        x = bp.int_image(*shape, 9)
        if whole:
            x[:] = float("-inf")
        else:
            x[:, :, :2, :2] = float("-inf")
            x[:, :, -1:, -2:] = float("-inf")
        if pre:
            # with the BN + ReLU applied on load nothing is -inf after the ReLU: scale 1 / shift 0 keeps relu(x) = 0
            # for every -inf, so all taps tie at 0 and the first in-bounds tap must win as well
            _maxpool_check(x, k, s, p, False, pre=torch.cat([torch.ones(shape[1]), torch.zeros(shape[1])]))
        else:
            _maxpool_check(x, k, s, p, False)


def test_4x4_minus_inf_gradient_lands_where_torch_puts_it():
    from bigdl_amd.ops import pool

    x = torch.full((1, 8, 4, 4), float("-inf"), dtype=BF).contiguous(memory_format=CL)
    y, idx = pool.maxpool_fwd_gpu(x.to(DEV), 3, 3, 2, 2, 1, 1)
    assert idx.cpu()[0, 0].reshape(-1).tolist() == [4, 3, 1, 0]
    dy = torch.tensor([[1.0, 2.0], [3.0, 5.0]]).expand(1, 8, 2, 2).to(BF).contiguous(memory_format=CL)
    dx = pool.maxpool_bwd_gpu(dy.to(DEV), idx, x.shape, 3, 3, 2, 2, 1, 1)
    xs = x.float().requires_grad_(True)
    torch.nn.functional.max_pool2d(xs, 3, 2, 1).backward(dy.float())
    assert torch.equal(dx.cpu().float(), xs.grad)
    assert dx.cpu()[0, 0, :2, :2].reshape(-1).tolist() == [1.0, 2.0, 3.0, 5.0]


@pytest.mark.parametrize("k,s,p", [(3, 2, 1), (2, 2, 0), (3, 1, 1)])
def test_nan_wins_and_the_last_nan_is_stored(k, s, p):
    x = bp.int_image(2, 8, 6, 6, 11)
    x[(torch.arange(x.numel()).view(x.shape) % 13) == 0] = float("nan")
    _maxpool_check_nan(x, k, s, p)


def _maxpool_check_nan(x, k, s, p):
    from bigdl_amd.ops import pool

    y_ref, idx_ref = bp.maxpool_oracle(x.float(), k, s, p)
    y, idx = pool.maxpool_fwd_gpu(x.to(DEV).contiguous(memory_format=CL), k, k, s, s, p, p)
    assert torch.equal(y.cpu().isnan(), y_ref.isnan()) and y_ref.isnan().any() and not y_ref.isnan().all()
    keep = ~y_ref.isnan()
    assert torch.equal(y.cpu().float()[keep], y_ref[keep])
    assert torch.equal(idx.cpu(), idx_ref)


if __name__ == "__main__":
    assert sys.argv[1:] == ["--exact-subset"]
    import bigdl_amd  # noqa: F401  (the HIP runtime settings, as tests/conftest.py)

    _exact_subset()
    print(f"exact subset ok U={os.environ.get('BIGDL_BN_UNROLL', '4')}")
