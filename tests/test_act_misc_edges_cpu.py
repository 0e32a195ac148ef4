"""tests/act_misc_edge_cases.py on its own, no GPU: the oracles against independent forms (torch.nn.functional and torch
autograd in fp64, the numpy Philox of tests/recurrent_cases.py and the published Philox test vectors, the CPU engine of
ops/nnk.py), the bounds against a correctly rounded result, and, with planted errors, that each comparison function the
GPU file uses rejects what it must."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import act_misc_edge_cases as am  # noqa: E402

BF, F32, F64 = am.BF, am.F32, am.F64
NAN = float("nan")


def _torch_form(kind, x, a, b):
    return {
        "Tanh": torch.tanh, "Sigmoid": torch.sigmoid, "ELU": lambda t: F.elu(t, a), "LeakyReLU": lambda t: F.leaky_relu(t, a),
        "ReLU6": lambda t: torch.clamp(t, 0.0, 6.0), "SoftPlus": lambda t: F.softplus(t, a, 20.0), "SoftSign": F.softsign,
        "HardTanh": lambda t: torch.clamp(t, a, b), "HardSigmoid": lambda t: torch.clamp(0.2 * t + 0.5, 0, 1),
        "LogSigmoid": F.logsigmoid, "TanhShrink": F.tanhshrink, "SoftShrink": lambda t: F.softshrink(t, a),
        "HardShrink": lambda t: F.hardshrink(t, a), "Threshold": lambda t: F.threshold(t, a, b), "Exp": torch.exp,
        "Log": torch.log, "Sqrt": torch.sqrt, "Square": torch.square, "Abs": torch.abs}[kind](x)


# ================================================================================================== activations
@pytest.mark.parametrize("kind", list(am.ACT))
def test_act_oracle_matches_torch_and_autograd(kind):
    """act_f64 == torch's own form in fp64; act_df64 (from x and the oracle's y) == fp64 autograd of it; the fp64 value
    rounded to fp32 / bf16 lies inside the bound with ratio <= 1 (a correctly rounded result passes)."""
    _, a, b = am.ACT[kind]
    x = am.act_gauss(kind, 1001, 3, F32).to(F64)
    if kind in am.ACT_EXP:
        x = x.clamp(-80, 80)
    y = am.act_f64(kind, x, a, b)
    xr = x.clone().requires_grad_(True)
    yt = _torch_form(kind, xr, a, b)
    assert torch.allclose(y, yt.detach(), rtol=1e-13, atol=1e-300), kind
    dy = torch.randn(1001, generator=am.gen(4)).to(F64)
    yt.backward(dy)
    assert torch.allclose(dy * am.act_df64(kind, x, y, a, b), xr.grad, rtol=1e-7, atol=1e-13), kind
    for dt in (F32, BF):
        assert am.elem_ratio(am.rnd(y, dt), y, am.act_bound(kind, x, a, b)) <= 1.0, (kind, dt)
        dx = dy * am.act_df64(kind, x, y, a, b)
        assert am.elem_ratio(am.rnd(dx, dt), dx, am.act_dbound(kind, x, y, dy, a, b)) <= 1.0, (kind, dt)


@pytest.mark.parametrize("kind", list(am.ACT))
def test_nan_rule_is_what_the_oracle_gives(kind):
    _, a, b = am.ACT[kind]
    keeps, dfn, _ = am.NAN_RULE[kind]
    x = torch.tensor([NAN], dtype=F64)
    y = am.act_f64(kind, x, a, b)
    assert bool(torch.isnan(y)) == keeps, kind
    df = am.act_df64(kind, x, y, a, b)
    want = {"nan": NAN, "a": a}.get(dfn, dfn)
    assert (torch.isnan(df).item() and want != want) or float(df) == want, (kind, float(df))


def _layer(kind):
    from bigdl_amd import nn

    _, a, b = am.ACT[kind]
    args = {"ELU": (a,), "LeakyReLU": (a,), "SoftPlus": (a,), "HardTanh": (a, b), "SoftShrink": (a,), "HardShrink": (a,),
            "Threshold": (a, b)}.get(kind, ())
    return getattr(nn, kind)(*args)


@pytest.mark.parametrize("kind", list(am.ACT))
def test_cpu_layers_and_nan(kind):
    """The CPU engine's ``fn`` of every layer on a NaN among numbers: NaN where NAN_RULE keeps it, the numbers within
    the forward bound. Pinned deviation: SoftShrink / HardShrink give 0 in the kernel and the reference, but NaN here
    (torch.nn.functional keeps it)."""
    _, a, b = am.ACT[kind]
    x = torch.tensor([NAN, 1.0, 0.5, 7.0, NAN])
    got = _layer(kind).forward(x)
    want = am.act_f64(kind, x, a, b)
    if kind in ("SoftShrink", "HardShrink"):
        assert not am.NAN_RULE[kind][0] and bool(torch.isnan(got[[0, 4]]).all()) and not bool(torch.isnan(want).any())
        got, want, x = got[1:4], want[1:4], x[1:4]
    else:
        assert am.NAN_RULE[kind][0] and torch.equal(torch.isnan(got), torch.isnan(x))
    assert am.elem_ratio(got, want, am.act_bound(kind, x, a, b)) <= am.ACT_CAP[kind], kind


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_edge_tables_and_exact_comparison(dtype):
    """The table holds each threshold and both neighbours in the dtype; a cyclic fill of 8 x len entries puts every
    entry at every position of a granule. Planted: one ulp, a threshold moved by one ulp, a cleaned NaN, a dropped tail
    element: each rejected by exact_equal."""
    for kind in am.ACT_EXACT:
        _, a, b = am.ACT[kind]
        tab = am.act_edge_table(kind, dtype, a, b)
        L = tab.numel()
        assert L % 2 == 1 and int(torch.isnan(tab).sum()) == 4
        for t in am.act_thresholds(kind, a, b):
            th = torch.tensor([t], dtype=dtype)
            for v in (th, am._next(th, True), am._next(th, False)):
                assert bool((am.bits(tab) == am.bits(v)).any()), (kind, t)
        up = am._next(torch.tensor([1.0], dtype=dtype), True)
        assert float(up) == 1 + (2.0 ** -23 if dtype == F32 else 2.0 ** -7)
        x = am.cyclic(tab, 8 * L + 5)
        pos = {(int(i) % L, int(i) % 8) for i in range(8 * L)}
        assert len(pos) == 8 * L
        want = am.act_f64(kind, x, a, b)
        good = am.rnd(want, dtype)
        assert am.exact_equal(good, want), kind
        fin = torch.isfinite(good) & (good != 0)
        i = int(torch.nonzero(fin)[3])
        bad = good.clone()
        bad[i] = am._next(good[i:i + 1], True)[0]                          # one ulp of the dtype
        assert not am.exact_equal(bad, want), kind
        bad = good.clone()
        bad[-1] = 0.0 if float(good[-1]) != 0.0 or torch.isnan(good[-1]) else 1.0   # dropped tail element
        assert not am.exact_equal(bad, want), kind
        if am.NAN_RULE[kind][0]:
            bad = torch.where(torch.isnan(good), torch.zeros_like(good), good)      # cleaned NaN
            assert not am.exact_equal(bad, want), kind
            assert am.elem_ratio(bad, want, torch.ones_like(want)) == float("inf")
        if kind != "Abs":
            # a threshold moved up by one ulp: the element one ulp above it falls on the other side of the compare
            t = {"ReLU6": 6.0, "HardTanh": b, "LeakyReLU": 0.0}.get(kind, a)
            e = am._next(torch.tensor([t], dtype=dtype), True)
            other = {"LeakyReLU": a * e.to(F64), "ReLU6": e.to(F64), "HardTanh": e.to(F64), "SoftShrink": 0.0 * e.to(F64),
                     "HardShrink": 0.0 * e.to(F64), "Threshold": b + 0.0 * e.to(F64)}[kind]
            at = am.bits(x) == am.bits(e)
            assert bool(at.any())
            moved = torch.where(at, other, want)
            assert not am.exact_equal(am.rnd(moved, dtype), want), kind


def test_hardsigmoid_clamp_ends():
    for dtype in (F32, BF):
        tab = am.act_edge_table("HardSigmoid", dtype)
        x = tab[torch.isfinite(tab)]
        df = am.act_df64("HardSigmoid", x, x)
        inside = (x.to(F64) >= -2.5) & (x.to(F64) <= 2.5)
        assert torch.equal(df != 0, inside) and bool((df[inside] == am.f32v(0.2)).all())


# ================================================================================================== LRN
@pytest.mark.parametrize("size,C", [(1, 1), (3, 2), (5, 13), (4, 13), (7, 6)])
def test_lrn_oracle_matches_cpu_engine_and_autograd(size, C):
    from bigdl_amd.ops import nnk

    alpha, beta, k = size * 0.0625, 0.75, 2.0
    x = torch.randn(2, C, 3, 5, generator=am.gen(size * 31 + C), dtype=F64).requires_grad_(True)
    y, s = am.lrn_oracle(x.detach(), size, alpha, beta, k)
    yc = nnk.lrn_cpu(x, size, alpha, beta, k)
    assert torch.allclose(y, yc.detach(), rtol=1e-12)
    gy = torch.randn(y.shape, generator=am.gen(9), dtype=F64)
    yc.backward(gy)
    gx, mag = am.lrn_bwd_oracle(x.detach(), y, s, gy, size, alpha, beta)
    assert torch.allclose(gx, x.grad, rtol=1e-10, atol=1e-13) and bool((mag >= gx.abs() * (1 - 1e-12)).all())
    assert am.elem_ratio(y.to(F32), y, am.lrn_y_bound(y, s, beta)) <= 1.0


def test_lrn_shifted_window_is_rejected():
    """A window one channel off: the exact scale leg is unequal, y misses its bound."""
    size, C = 5, 13
    x = am.lrn_int(2, C, 1, 7, 5)
    y, s = am.lrn_oracle(x, size, size * 0.0625, 0.75, 1.0)
    assert am.st.is_f32(s)
    xs = torch.roll(x, 1, 1)
    xs[:, 0] = 0
    ys, ss = am.lrn_oracle(xs, size, size * 0.0625, 0.75, 1.0)        # scale of window [c - pre - 1, ...]
    assert not torch.equal(ss.to(F32), s.to(F32))
    bad = (x.to(F64) * ss.pow(-0.75)).to(F32)
    assert am.elem_ratio(bad, y, am.lrn_y_bound(y, s, 0.75)) > 8.0


def test_lrn_dynamic_range_bound_covers_fp32_running_sum():
    """The running window in fp32 on the CPU (adds and subtractions in the kernel's order) stays inside the chain
    bound, and the bound is far below the 1e8 the large channel contributes (so a lost channel is seen)."""
    size, C = 5, 9
    for pos in range(C):
        x = torch.full((1, C, 1, 4), 1e-2)
        x[:, pos] = 1e4
        _, s = am.lrn_oracle(x, size, size * 0.0625, 0.75, 1.0)
        bound = am.lrn_scale_chain_bound(x, size, size * 0.0625, 1.0)
        pre, win, got = (size - 1) // 2, torch.zeros(1, 1, 4), torch.empty_like(x)
        for c in range(min(size - pre - 1, C)):
            win = win + x[:, c] * x[:, c]
        for c in range(C):
            if c + size - pre - 1 < C:
                win = win + x[:, c + size - pre - 1] ** 2
            if c - pre - 1 >= 0:
                win = win - x[:, c - pre - 1] ** 2
            got[:, c] = 1.0 + 0.0625 * win.clamp_min(0)
        assert bool(((got.to(F64) - s).abs() <= bound).all()) and bool((got >= 1.0).all())
        assert float(bound.max()) < 1e3


# ================================================================================================== dropout
def test_philox_published_vectors_and_numpy_oracle():
    """Random123 kat_vectors for philox4x32-10, then the kernel's layout against tests/recurrent_cases.py."""
    kat = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))
    for ctr, key, want in kat:
        r = am.philox4x32([torch.tensor([c]) for c in ctr], [torch.tensor([k]) for k in key])
        assert tuple(int(v) for v in r) == want
    for seed in am.DROPOUT_SEEDS:
        ids = np.arange(1003, dtype=np.uint64)
        r_np = am._philox_np(seed, ids >> np.uint64(2))
        q = torch.arange(1003) >> 2
        z = torch.zeros_like(q)
        r_t = am.philox4x32((q, z, z, z), (z + (seed & am.M32), z + (seed >> 32)))
        assert all(np.array_equal(a.astype(np.int64), b.numpy()) for a, b in zip(r_np, r_t)), seed
        for p in (0.0, 0.3, 0.5, 1.0):
            assert np.array_equal(am._keep_mask(seed, ids, am.f32v(p)), am.dropout_keep(seed, 1003, p).numpy()), (seed, p)


def test_dropout_planted_stream_errors_are_rejected():
    seed, n = 2 ** 32 + 12345, 1003
    x = am.dropout_input(n, 7, F32)
    want = am.dropout_oracle(x, am.dropout_keep(seed, n, 0.5), 2.0)
    for swap in ("lane", "counter", "key"):
        bad = am.dropout_oracle(x, am.dropout_keep(seed, n, 0.5, swap=swap), 2.0)
        assert not am.same_bits_nan(bad, want), swap
    assert bool(am.dropout_keep(seed, n, 0.0).all()) and not bool(am.dropout_keep(seed, n, 1.0).any())
    # u == 0 is one draw in 2^24: DROPOUT_ZERO_DRAW names one, where '>' in place of '>=' drops the element at p = 0
    zs, zi = am.DROPOUT_ZERO_DRAW
    k, g = am.dropout_keep(zs, zi + 1, 0.0), am.dropout_keep(zs, zi + 1, 0.0, swap="gt")
    assert bool(k.all()) and not bool(g[zi]) and bool(g[:zi].all())


def test_dropout_oracle_values():
    x = torch.tensor([NAN, float("inf"), -0.0, 1.5, NAN, -float("inf")])
    keep = torch.tensor([True, True, True, True, False, False])
    for dt in (F32, BF):
        y = am.dropout_oracle(x.to(dt), keep, 2.0)
        assert torch.isnan(y[0]) and float(y[1]) == float("inf") and float(y[3]) == 3.0
        assert am.same_bits(y[2:3], torch.tensor([-0.0], dtype=dt)) and am.same_bits(y[4:], torch.zeros(2, dtype=dt))
    xb = torch.tensor([1.0 + 2.0 ** -7], dtype=BF)                      # x 1.5 = 1.51171875: a bf16 tie, to even
    assert float(am.dropout_oracle(xb, keep[:1], 1.5)) == 1.515625


# ================================================================================================== embedding
def test_embedding_oracles_and_planted_errors():
    W = torch.randn(7, 5, generator=am.gen(1))
    ids = am.emb_ids(9, 7, 2, F32)
    out = am.emb_fwd_oracle(W, ids, True)
    k = ids.long() - 1
    for r in range(9):
        want = W[k[r]] if 0 <= k[r] < 7 else torch.zeros(5)
        assert torch.equal(out[r], want)
    assert torch.equal(am.emb_fwd_oracle(W, torch.tensor([0.0, -2.0]), False), W[[0, 0]])
    shifted = am.emb_fwd_oracle(W, ids + 1, True)                        # row taken from id + 1
    assert not am.same_bits(shifted, out)
    g = torch.randint(-4, 5, (9, 5), generator=am.gen(3)).float()
    gW0 = torch.randint(-4, 5, (7, 5), generator=am.gen(4)).float()
    keys = am.emb_keys(ids, 3)
    got, mag, run = am.emb_bwd_oracle(gW0, keys, g, 0.5)
    ref = gW0.to(F64).clone()
    for r in range(9):
        if 0 <= keys[r] < 7:
            ref[keys[r]] += 0.5 * g[r].to(F64)
    assert torch.equal(got, ref) and am.st.is_f32(got) and int(run.sum()) == int(((keys >= 0) & (keys < 7)).sum())
    assert bool((keys != 3).all())
    r_ok = int(torch.nonzero((keys >= 0) & (keys < 7))[0])
    twice, _, _ = am.emb_bwd_oracle(gW0, keys, g, 0.5, twice=r_ok)
    assert not torch.equal(twice.to(F32), got.to(F32))


# ================================================================================================== resize
@pytest.mark.parametrize("align", [False, True])
def test_resize_oracle_matches_cpu_engine_and_autograd(align):
    from bigdl_amd.ops import nnk

    for H, W, OH, OW in am.RESIZE_GEO + ((10, 3, 30, 9),):
        x = torch.randn(2, 3, H, W, generator=am.gen(H * 100 + OW), dtype=F64).requires_grad_(True)
        y, mag = am.resize_oracle(x.detach(), OH, OW, align)
        yc = nnk.resize_bilinear_cpu(x, OH, OW, align)
        assert torch.allclose(y, yc.detach(), rtol=1e-12, atol=1e-12), (H, W, OH, OW)
        gy = torch.randn(y.shape, generator=am.gen(5), dtype=F64)
        yc.backward(gy)
        gx, gm, cnt = am.resize_bwd_oracle(gy, H, W, align)
        assert torch.allclose(gx, x.grad, rtol=1e-11, atol=1e-12), (H, W, OH, OW)
        assert float(cnt.sum()) == 4 * y.numel()
        assert am.elem_ratio(y.to(F32), y, am.ulp32(mag)) <= 1.0


def test_resize_integer_landings_and_moved_floor():
    """3 -> 9 and 5 -> 7: o x fp32(in / out) lands on an integer for some o (3 x fp32(1/3) == 1.0f); a floor moved by one
    there changes the result beyond the bound."""
    s = torch.arange(9, dtype=F32) * torch.tensor(3 / 9, dtype=F32)
    assert s[3] == 1.0 and s[6] == 2.0 and float(torch.tensor(3 / 9, dtype=F32)) * 3 > 1.0
    s = torch.arange(7, dtype=F32) * torch.tensor(5 / 7, dtype=F32)          # 5 -> 7: no interior landing, o = 0 only
    assert int((s == s.floor()).sum()) == 1
    x = torch.randn(1, 2, 3, 3, generator=am.gen(8))
    y, mag = am.resize_oracle(x, 9, 9, False)
    bad, _ = am.resize_oracle(x, 9, 9, False, floor_shift=1)
    assert am.elem_ratio(bad.to(F32), y, am.ulp32(mag)) > 4.0


# ================================================================================================== log-softmax
def test_log_softmax_oracle_bound_and_planted_errors():
    x = am.lsm_gauss(5, 65, 4.0, 0.0, 3)
    y = am.lsm_oracle(x)
    assert am.elem_ratio(torch.log_softmax(x, 1), y, am.lsm_bound(x)) <= 4.0
    assert am.elem_ratio(am.lsm_oracle(x, skip_last=True).to(F32), y, am.lsm_bound(x)) > 4.0
    xr = x.to(F64).requires_grad_(True)
    gy = torch.randn(5, 65, generator=am.gen(4), dtype=F64)
    torch.log_softmax(xr, 1).backward(gy)
    gx, bound = am.lsm_bwd_oracle(y, gy)
    assert torch.allclose(gx, xr.grad, rtol=1e-11, atol=1e-13)
    assert am.elem_ratio(gx.to(F32), gx, bound) <= 1.0
    xi = x.clone()
    xi[1] = -float("inf")
    xi[2, 0] = -float("inf")
    xi[3, 7] = float("inf")
    yi = am.lsm_oracle(xi)
    t = torch.log_softmax(xi, 1)
    assert torch.equal(torch.isnan(yi), torch.isnan(t)) and bool(torch.isnan(yi[1]).all()) and bool(torch.isnan(yi[3]).all())
    assert float(yi[2, 0]) == -float("inf") and am.elem_ratio(t, yi, am.lsm_bound(xi)) <= 4.0
    assert float(am.lsm_oracle(torch.tensor([[3.0], [-2.0]])).abs().max()) == 0.0


# ================================================================================================== canaries
def test_guarded_view_sees_a_byte_outside():
    for dt, off in ((F32, 1), (BF, 7)):
        v, full, lead = am.guarded(9, dt, "cpu", off)
        v.fill_(1.0)
        nb = 9 * v.element_size()
        assert am.canaries_ok(full, lead, nb) and (lead - 256) == off * v.element_size()
        for at in (lead - 1, lead + nb):
            full[at] ^= 1
            assert not am.canaries_ok(full, lead, nb)
            full[at] ^= 1
