"""The point-wise activation kernels (csrc/activation.hip) and the misc NN kernels (csrc/nn_misc.hip), each through its
own binding, against the oracles of tests/act_misc_edge_cases.py: act_fwd / act_bwd (19 kinds x fp32 / bf16), lrn_fwd /
lrn_bwd, dropout, embedding_fwd / _fwd_ids / _bwd / _bwd_ids (atomic and sorted routes), resize_bilinear_fwd / _bwd,
log_softmax_fwd / _bwd.

* exact legs are held to equality with the fp64 oracle rounded once (NaN positions, signed zeros), never to another
  launch of a kernel, except where two launches must be bitwise equal;
* element-wise legs are held to ``allowed x bound`` per element; the largest ratios measured on an MI355X and the allowed
  values taken from them (``ALLOWED``) are in profiles/act_misc_edge_errors.txt;
* every tensor a kernel touches is a view inside a larger allocation of sentinel bytes (``_Arena``); views at element
  offsets 0-3 (fp32) and 0, 1, 4, 7 (bf16) reach the scalar routes the host functions choose by alignment.
"""
import contextlib
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import act_misc_edge_cases as am  # noqa: E402

pytestmark = pytest.mark.gpu

BF, F32, F64 = am.BF, am.F32, am.F64
DEV = "cuda"
DTS = [F32, BF]
DT_IDS = ["f32", "bf16"]
OFFS = {F32: (0, 1, 2, 3), BF: (0, 1, 4, 7)}

# Caps fixed before measuring: 4 for one rounded operation chain, 8 where a fast intrinsic (__expf, __logf, __powf) feeds
# further arithmetic, 1 for worst-case chain bounds. Allowed = 2 x the largest ratio measured on an MI355X, rounded up,
# never above the cap (profiles/act_misc_edge_errors.txt). bf16 results add half a bf16 spacing to the bound.
CAPS = {"act_fwd": dict(am.ACT_CAP), "act_bwd": dict(am.ACT_CAP), "lrn_y": 8.0, "lrn_gx": 1.0, "lrn_range": 1.0,
        "emb_det": 1.0, "resize_fwd": 4.0, "resize_bwd": 1.0, "lsm_fwd": 4.0, "lsm_bwd": 1.0}
_EXACT0 = {k: 0.0 for k in am.ACT_EXACT}       # exact on Gaussian data too (measured 0): nothing is allowed
# fp32 figures: each from the largest fp32 ratio (the bf16 maxima, 0.985 = 1 / (1 + 2^-6) for every kind, are held to 1)
ALLOWED = {"act_fwd": dict(_EXACT0, Tanh=2.3, Sigmoid=4.2, ELU=0.73, SoftPlus=2.3, SoftSign=2.5, HardSigmoid=1.2,
                           LogSigmoid=2.6, TanhShrink=2.3, Exp=2.4, Log=4.1, Sqrt=1.0, Square=1.0),
           "act_bwd": dict(_EXACT0, Tanh=1.3, Sigmoid=3.4, ELU=1.2, SoftPlus=4.3, SoftSign=4.0, HardSigmoid=1.6,
                           LogSigmoid=4.3, TanhShrink=3.3, Exp=1.9, Log=2.5, Sqrt=2.5, Square=1.8),
           "lrn_y": 2.3, "lrn_gx": 1.0, "lrn_range": 0.23, "emb_det": 0.55, "resize_fwd": 3.1, "resize_bwd": 1.0,
           "lsm_fwd": 1.9, "lsm_bwd": 1.0}
assert set(ALLOWED["act_fwd"]) == set(am.ACT) == set(ALLOWED["act_bwd"])


def _allowed(leg, kind=None, dtype=F32):
    """A bf16 result is held to the bound as derived (the fp32 bound + half a bf16 spacing): allowed ratio 1."""
    a, c = ALLOWED[leg], CAPS[leg]
    a, c = (a[kind], c[kind]) if kind else (a, c)
    assert a <= c
    return (1.0 if a > 0 else 0.0) if dtype == BF else a


def _report(leg, case, value):
    print(f"ACT_MISC|{leg}|{case}|{value:.4g}")
    return value


def _n():
    from bigdl_amd.ops import native

    return native.get()


@contextlib.contextmanager
def _det(on):
    from bigdl_amd.ops import native

    _n()
    old = native.deterministic()
    native.set_deterministic(on)
    try:
        yield
    finally:
        native.set_deterministic(old)


class _Arena:
    """Guarded device views; ``ok()`` after the launches asserts every sentinel byte on both sides of every view."""

    def __init__(self):
        self.items = []

    def new(self, n, dtype, off=0, shape=None):
        v, full, lead = am.guarded(n, dtype, DEV, off)
        assert full.data_ptr() % 256 == 0
        self.items.append((full, lead, n * v.element_size()))
        return v if shape is None else v.view(shape)

    def put(self, src, off=0):
        v = self.new(src.numel(), src.dtype, off)
        v.copy_(src.reshape(-1))
        return v.view(src.shape)

    def ok(self):
        torch.cuda.synchronize()
        return all(am.canaries_ok(*it) for it in self.items)


# ================================================================================================== activations
def _act_fwd(kind, x, ox=0, oy=0):
    code, a, b = am.ACT[kind]
    ar = _Arena()
    xd, y = ar.put(x, ox), ar.new(x.numel(), x.dtype, oy, x.shape)
    _n().act_fwd(xd, y, code, a, b)
    assert ar.ok(), ("canary", kind, x.numel(), ox, oy)
    return y


def _act_bwd(kind, x, y, dy, offs=(0, 0, 0, 0)):
    code, a, b = am.ACT[kind]
    ar = _Arena()
    xd, yd, gd = ar.put(x, offs[0]), ar.put(y, offs[1]), ar.put(dy, offs[2])
    dx = ar.new(x.numel(), x.dtype, offs[3], x.shape)
    _n().act_bwd(xd, yd, gd, dx, code, a, b)
    assert ar.ok(), ("canary", kind, x.numel(), offs)
    return dx


def _act_exact_case(kind, x, seed, tag, ox=0, oy=0, offs=(0, 0, 0, 0)):
    _, a, b = am.ACT[kind]
    want = am.act_f64(kind, x, a, b)
    assert am.exact_equal(_act_fwd(kind, x, ox, oy), want), ("fwd", kind, tag)
    y = am.rnd(want, x.dtype)                              # the y handed to the backward: the oracle's, rounded
    dy = am.int_dy(x.numel(), seed, x.dtype)
    dxw = dy.to(F64) * am.act_df64(kind, x, y, a, b)
    assert am.exact_equal(_act_bwd(kind, x, y, dy, offs), dxw), ("bwd", kind, tag)


@pytest.mark.parametrize("dtype", DTS, ids=DT_IDS)
@pytest.mark.parametrize("kind", am.ACT_EXACT)
def test_act_exact_edge_table(kind, dtype):
    """Piecewise-linear kinds and Abs: each threshold and one ulp either side, +-0, +-inf, the largest finite value,
    denormals and four NaN at every position of a 16-byte granule and in the scalar tail, forward and backward by bits.
    This is also where the NaN rule and the closed-interval gradient at the clamp bounds are pinned."""
    _, a, b = am.ACT[kind]
    tab = am.act_edge_table(kind, dtype, a, b)
    L = tab.numel()
    for n in am.ACT_N:
        shifts = range(0, L, 7) if n <= 17 else (0, 3)
        for s in shifts:
            _act_exact_case(kind, am.cyclic(tab, n, s), n + s, (n, s))
    x = torch.tensor([float("nan")] * 9, dtype=dtype)
    y = _act_fwd(kind, x)
    assert bool(torch.isnan(y).all()) == am.NAN_RULE[kind][0] and bool((torch.isnan(y) | (y == 0)).all()), kind


@pytest.mark.parametrize("dtype", DTS, ids=DT_IDS)
def test_act_square_integers_and_hardsigmoid_ends(dtype):
    x = torch.randint(-9, 10, (1001,), generator=am.gen(3)).to(dtype)
    _act_exact_case("Square", x, 5, "int")
    tab = am.act_edge_table("HardSigmoid", dtype)
    x = am.cyclic(tab, 8 * tab.numel() + 5)
    want = am.act_f64("HardSigmoid", x)
    r = _report("act_fwd", f"HardSigmoid ends {DT_IDS[DTS.index(dtype)]}", am.elem_ratio(_act_fwd("HardSigmoid", x), want,
                                                                     am.act_bound("HardSigmoid", x)))
    assert r <= _allowed("act_fwd", "HardSigmoid", dtype)
    dy = (am.int_dy(x.numel(), 7, dtype).sign() * 4).to(dtype)          # 4 x fp32(0.2): exact in fp32
    dxw = dy.to(F64) * am.act_df64("HardSigmoid", x, am.rnd(want, dtype))
    assert am.exact_equal(_act_bwd("HardSigmoid", x, am.rnd(want, dtype), dy), dxw)


@pytest.mark.parametrize("dtype", DTS, ids=DT_IDS)
def test_act_alignment_offsets(dtype):
    """Views at element offsets inside a 256-byte aligned buffer, inputs and outputs independently: the host function
    takes the 16-byte body only when every pointer is aligned, the scalar loop otherwise. Exact (ReLU6 table)."""
    tab = am.act_edge_table("ReLU6", dtype)
    x = am.cyclic(tab, 1001)
    for ox in OFFS[dtype]:
        for oy in OFFS[dtype]:
            _, a, b = am.ACT["ReLU6"]
            assert am.exact_equal(_act_fwd("ReLU6", x, ox, oy), am.act_f64("ReLU6", x)), (ox, oy)
    for i in range(4):
        for o in OFFS[dtype][1:]:
            offs = [0, 0, 0, 0]
            offs[i] = o
            _act_exact_case("ReLU6", x, 11, ("off", i, o), offs=tuple(offs))
    for o in OFFS[dtype][1:]:
        _act_exact_case("ReLU6", x, 12, ("all", o), o, o, (o, o, o, o))


def _act_elem_case(kind, x, seed, tag):
    _, a, b = am.ACT[kind]
    want = am.act_f64(kind, x, a, b)
    rf = _report("act_fwd", f"{kind} {tag}", am.elem_ratio(_act_fwd(kind, x), want, am.act_bound(kind, x, a, b)))
    y = am.rnd(want, x.dtype)
    dy = (torch.randn(x.shape, generator=am.gen(seed)) * 2).to(x.dtype)
    dxw = dy.to(F64) * am.act_df64(kind, x, y, a, b)
    rb = _report("act_bwd", f"{kind} {tag}", am.elem_ratio(_act_bwd(kind, x, y, dy), dxw,
                                                           am.act_dbound(kind, x, y, dy, a, b)))
    assert rf <= _allowed("act_fwd", kind, x.dtype) and rb <= _allowed("act_bwd", kind, x.dtype), (kind, tag, rf, rb)


@pytest.mark.parametrize("dtype", DTS, ids=DT_IDS)
@pytest.mark.parametrize("kind", list(am.ACT))
def test_act_elementwise(kind, dtype):
    """Gaussian data and a sweep of magnitudes 2^-20 .. 2^6 against fp64, forward and backward, per element; a dense
    channels-last 4-D tensor; SoftPlus around a x = 20 and where exp underflows; Sqrt(0) / Log(0) with the backward."""
    for n in am.ACT_N:
        _act_elem_case(kind, am.act_gauss(kind, n, 100 + n, dtype), n, f"n={n} {DT_IDS[DTS.index(dtype)]}")
    x = am.act_gauss(kind, 3 * 8 * 5 * 7, 9, dtype).view(3, 8, 5, 7)
    code, a, b = am.ACT[kind]
    ar = _Arena()                                          # NHWC storage seen as NCHW: dense channels-last views
    xd, y = (ar.new(x.numel(), dtype).view(3, 5, 7, 8).permute(0, 3, 1, 2) for _ in range(2))
    xd.copy_(x)
    assert y.stride() == xd.stride() and not xd.is_contiguous() and xd.is_contiguous(memory_format=torch.channels_last)
    _n().act_fwd(xd, y, code, a, b)
    assert ar.ok()
    r = _report("act_fwd", f"{kind} channels-last {DT_IDS[DTS.index(dtype)]}",
                am.elem_ratio(y.cpu(), am.act_f64(kind, x, a, b), am.act_bound(kind, x, a, b)))
    assert r <= _allowed("act_fwd", kind, dtype)
    if kind == "SoftPlus":
        t = torch.tensor([10.0], dtype=dtype)
        x = torch.cat([am._next(t, False), t, am._next(t, True), torch.tensor([-40.0, -52.0, -60.0, -200.0], dtype=dtype)])
        _act_elem_case(kind, x, 1, f"around a x = 20 {DT_IDS[DTS.index(dtype)]}")
    if kind in ("Sqrt", "Log"):
        x = torch.tensor([0.0, 1.0, 4.0], dtype=dtype)
        _act_elem_case(kind, x, 1, f"at 0 {DT_IDS[DTS.index(dtype)]}")


@pytest.mark.parametrize("dtype", DTS, ids=DT_IDS)
@pytest.mark.parametrize("kind", ["ReLU6", "Sigmoid"])
def test_act_second_grid_stride_trip(kind, dtype):
    """8192 x 256 x 8 + 11 elements: the vector body's second trip, tail present; compared on the device."""
    code, a, b = am.ACT[kind]
    n = am.ACT_PAST_CAP
    g = torch.Generator(device=DEV).manual_seed(5)
    ar = _Arena()
    x = ar.new(n, dtype)
    x.copy_(torch.randn(n, device=DEV, generator=g) * 3)
    x[-11:] = torch.tensor([7.0, -1, 0.5, float("nan"), 6, -0.0, 3, 9, -7, 2, 100], dtype=dtype, device=DEV)
    y, dx = ar.new(n, dtype), ar.new(n, dtype)
    _n().act_fwd(x, y, code, a, b)
    want = am.act_f64(kind, x, a, b)
    yo = ar.put(am.rnd(want, dtype))
    dy = ar.new(n, dtype)
    dy.copy_(torch.randint(1, 5, (n,), device=DEV, generator=g))
    _n().act_bwd(x, yo, dy, dx, code, a, b)
    dxw = dy.to(F64) * am.act_df64(kind, x, yo, a, b)
    assert ar.ok()
    if kind == "ReLU6":
        nb = torch.isnan(yo)
        assert torch.equal(torch.isnan(y), nb) and torch.equal(y.masked_fill(nb, 0), yo.masked_fill(nb, 0))
        assert torch.equal(dx, am.rnd(dxw, dtype))
    else:
        rf = _report("act_fwd", f"{kind} past cap {DT_IDS[DTS.index(dtype)]}", am.elem_ratio(y, want, am.act_bound(kind, x, a, b)))
        rb = _report("act_bwd", f"{kind} past cap {DT_IDS[DTS.index(dtype)]}", am.elem_ratio(dx, dxw, am.act_dbound(kind, x, yo, dy, a, b)))
        assert rf <= _allowed("act_fwd", kind, dtype) and rb <= _allowed("act_bwd", kind, dtype)


@pytest.mark.parametrize("dtype", DTS, ids=DT_IDS)
@pytest.mark.parametrize("kind", list(am.ACT))
def test_act_nan_rule_every_kind(kind, dtype):
    """Nine NaN (one granule + the tail) and the four NaN patterns among numbers, through every kind: the forward keeps
    the NaN or gives +0 as NAN_RULE says; the backward, on the oracle's y and integer dy, gives NaN or dy x the
    pinned factor (by bits, the sign of a zero product included)."""
    _, a, b = am.ACT[kind]
    keeps, dfn, _ = am.NAN_RULE[kind]
    tab = am.act_edge_table("Abs", dtype)
    nans = tab[torch.isnan(tab)]
    assert nans.numel() == 4
    for x in (nans.repeat(3)[:9], torch.cat([torch.tensor([1.0, 2.0, 0.5], dtype=dtype), nans, nans, nans])):
        isn = torch.isnan(x)
        y = _act_fwd(kind, x).cpu()
        want = am.act_f64(kind, x, a, b)
        assert torch.equal(torch.isnan(y), isn if keeps else torch.zeros_like(isn)), kind
        assert keeps or am.same_bits(y[isn], torch.zeros_like(y[isn])), kind
        assert am.elem_ratio(y, want, am.act_bound(kind, x, a, b)) <= _allowed("act_fwd", kind, dtype), kind
        yo = am.rnd(want, dtype)
        dy = am.int_dy(x.numel(), 3, dtype)
        dx = _act_bwd(kind, x, yo, dy).cpu()
        if dfn == "nan":
            assert bool(torch.isnan(dx[isn]).all()), kind
        else:
            fac = a if dfn == "a" else dfn
            assert am.same_bits(dx[isn], am.rnd(dy[isn].to(F64) * fac, dtype)), kind
        dxw = dy.to(F64) * am.act_df64(kind, x, yo, a, b)
        assert am.elem_ratio(dx, dxw, am.act_dbound(kind, x, yo, dy, a, b)) <= _allowed("act_bwd", kind, dtype), kind


def test_act_ulps_near_zero_information():
    """ELU and TanhShrink near x = 0, in ulps of the result (printed, not asserted: the bound is at the largest term)."""
    for kind in ("ELU", "TanhShrink"):
        _, a, b = am.ACT[kind]
        x = -(2.0 ** torch.arange(-20, -2).float())
        y = _act_fwd(kind, x).cpu()
        want = am.act_f64(kind, x, a, b)
        _report("info_ulps_of_result", kind, float(((y.to(F64) - want).abs() / am.ulp32(want)).max()))


# ================================================================================================== LRN
def _lrn(x, size, alpha, beta, k):
    ar = _Arena()
    xd = ar.put(x)
    y, s = ar.new(x.numel(), F32, 0, x.shape), ar.new(x.numel(), F32, 0, x.shape)
    _n().lrn_fwd(xd, y, s, size, alpha, beta, k)
    assert ar.ok(), ("canary", tuple(x.shape), size)
    return y, s


def test_lrn_scale_exact():
    """Integer x, dyadic alpha / size and k: the scale output equals k + alpha_n sum x^2 over the clipped window."""
    for size, C in am.lrn_exact_geometry():
        for N, HW in ((1, 1), (2, 63), (1, 64), (2, 65)):
            x = am.lrn_int(N, C, 1, HW, size * 100 + C)
            _, s = _lrn(x, size, size * 0.0625, 0.75, 2.0)
            _, want = am.lrn_oracle(x, size, size * 0.0625, 0.75, 2.0)
            assert am.st.is_f32(want) and torch.equal(s.cpu().to(F64), want), (size, C, N, HW)


def test_lrn_elementwise_and_3d_module_path():
    from bigdl_amd.ops import nnk

    for size, C, beta, k in ((5, 13, 0.75, 1.0), (4, 13, 0.5, 2.0), (3, 2, 0.75, 2.0), (7, 6, 0.5, 1.0), (1, 1, 0.75, 1.0)):
        x = torch.randn(2, C, 5, 13, generator=am.gen(size + C))
        alpha = 1.0
        y, s = _lrn(x, size, alpha, beta, k)
        yw, sw = am.lrn_oracle(x, size, alpha, beta, k)
        r = _report("lrn_y", f"size={size} C={C} beta={beta}", am.elem_ratio(y.cpu(), yw, am.lrn_y_bound(yw, sw, beta)))
        assert r <= _allowed("lrn_y")
        yo, so = yw.to(F32), sw.to(F32)                        # the y / scale handed to the backward: the oracle's
        gy = torch.randn(x.shape, generator=am.gen(77))
        ar = _Arena()
        gx = ar.new(x.numel(), F32, 0, x.shape)
        _n().lrn_bwd(ar.put(x), ar.put(yo), ar.put(so), ar.put(gy), gx, size, alpha, beta)
        assert ar.ok()
        gw, mag = am.lrn_bwd_oracle(x, yo, so, gy, size, alpha, beta)
        r = _report("lrn_gx", f"size={size} C={C} beta={beta}",
                    am.elem_ratio(gx.cpu(), gw, am.lrn_gx_bound(mag, so.to(F64), size, beta)))
        assert r <= _allowed("lrn_gx")
    x = torch.randn(13, 5, 7, generator=am.gen(2))
    y3 = nnk.lrn(x.to(DEV), 5, 1.0, 0.75, 1.0)
    yw, sw = am.lrn_oracle(x[None], 5, 1.0, 0.75, 1.0)
    assert y3.shape == x.shape and am.elem_ratio(y3.cpu()[None], yw, am.lrn_y_bound(yw, sw, 0.75)) <= _allowed("lrn_y")


def test_lrn_dynamic_range():
    """One channel of 1e4 among channels of 1e-2, at each position: scale within the running sum's chain bound, never
    below k (the window sum is clamped at 0 after the large square leaves)."""
    size, C = 5, 9
    for pos in range(C):
        x = torch.full((1, C, 1, 65), 1e-2)
        x[:, pos] = 1e4
        _, s = _lrn(x, size, size * 0.0625, 0.75, 1.0)
        _, sw = am.lrn_oracle(x, size, size * 0.0625, 0.75, 1.0)
        r = _report("lrn_range", f"pos={pos}", am.elem_ratio(s.cpu(), sw, am.lrn_scale_chain_bound(x, size, size * 0.0625, 1.0)))
        assert r <= _allowed("lrn_range") and bool((s >= 1.0).all()), pos


def test_lrn_second_grid_stride_trip():
    """N x HW = 16384 x 256 + 1 columns, C = 2, size 3, integers: scale exact, on the device."""
    N, HW = 1, am.LRN_PAST_CAP_COLS
    x = torch.randint(-4, 5, (N, 2, 1, HW), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)).float()
    ar = _Arena()
    x = ar.put(x)
    y, s = ar.new(x.numel(), F32, 0, x.shape), ar.new(x.numel(), F32, 0, x.shape)
    _n().lrn_fwd(x, y, s, 3, 3 * 0.0625, 0.75, 2.0)
    assert ar.ok()
    sq = x.double() ** 2
    want = 2.0 + 0.0625 * (sq[:, 0] + sq[:, 1])                 # size 3, C = 2: both windows hold both channels
    assert torch.equal(s[:, 0].double(), want) and torch.equal(s[:, 1].double(), want)


# ================================================================================================== dropout
def _dropout(x, p, mul, seed):
    ar = _Arena()
    xd, y = ar.put(x), ar.new(x.numel(), x.dtype)
    _n().dropout(xd, y, p, mul, seed)
    assert ar.ok(), ("canary", x.numel(), p, seed)
    return y


@pytest.mark.parametrize("dtype", DTS, ids=DT_IDS)
def test_dropout_philox_stream_by_bits(dtype):
    """The keep mask equals the Philox-4x32-10 oracle bit for bit (counter = index / 4, lane = index % 4, key = the
    seed's halves), y = round(x * mul) where kept, +0 where dropped (NaN / inf included); the same call on dy gives
    the same mask; p = 0 keeps everything, p = 1 (mul = 1) nothing."""
    for seed in am.DROPOUT_SEEDS:
        for n in am.DROPOUT_N:
            x = am.dropout_input(n, n + 1, dtype)
            for p, mul in ((0.3, 1 / 0.7), (0.5, 2.0), (0.0, 1.5), (1.0, 1.0)):
                keep = am.dropout_keep(seed, n, p)
                y = _dropout(x, p, mul, seed).cpu()
                assert am.same_bits_nan(y, am.dropout_oracle(x, keep, mul)), (seed, n, p)
                assert p not in (0.0, 1.0) or bool(keep.all()) == (p == 0.0)
            dy = am.int_dy(n, 3, dtype)
            g = _dropout(dy, 0.5, 2.0, seed).cpu()
            assert torch.equal(g != 0, am.dropout_keep(seed, n, 0.5)), (seed, n)


def test_dropout_second_trip_grid_independence_and_zero_draw():
    """16384 x 256 x 4 + 5 elements: the mask on the device, its first 1003 elements against the oracle of the short
    launch; and the element whose uniform is exactly 0 is kept at p = 0 (u >= p)."""
    n, seed = am.DROPOUT_PAST_CAP, 2 ** 32 + 7
    ar = _Arena()
    x = ar.new(n, F32)
    x.fill_(1.0)
    y = ar.new(n, F32)
    _n().dropout(x, y, 0.5, 2.0, seed)
    assert ar.ok()
    keep = am.dropout_keep(seed, n, 0.5, device=DEV)
    assert torch.equal(y, torch.where(keep, 2.0, 0.0).float())
    assert torch.equal(y[:1003].cpu() != 0, am.dropout_keep(seed, 1003, 0.5))
    zs, zi = am.DROPOUT_ZERO_DRAW
    x = torch.arange(zi + 2, dtype=F32) + 1
    assert am.same_bits(_dropout(x, 0.0, 1.0, zs).cpu(), x)


def test_dropout_module_edges():
    from bigdl_amd import nn

    x = torch.randn(1003, device=DEV)
    m = nn.Dropout(1.0)
    m.training()
    y = m.forward(x)
    assert float(y.abs().max()) == 0.0 and float(m.backward(x, torch.ones_like(x)).abs().max()) == 0.0
    m = nn.Dropout(0.5)
    m.training()
    y = m.forward(x)
    keep = am.dropout_keep(m._seed & 0x7FFFFFFFFFFFFFFF, 1003, 0.5)
    assert am.same_bits(y.cpu(), am.dropout_oracle(x.cpu(), keep, 2.0))


# ================================================================================================== embedding
@pytest.mark.parametrize("ids_dt", [F32, torch.int64], ids=["ids-f32", "ids-i64"])
def test_embedding_forward_by_bits(ids_dt):
    C = _n()
    nIndex = 11
    for D in am.EMB_D:
        for rows in am.EMB_ROWS + (9,):
            W = torch.randn(nIndex, D, generator=am.gen(D))
            ids = am.emb_ids(rows, nIndex, rows + D, ids_dt)
            for mz in (False, True):
                for ow, oo in ((0, 0), (1, 0), (0, 2), (3, 3)):
                    ar = _Arena()
                    Wd, out = ar.put(W, ow), ar.new(rows * D, F32, oo, (rows, D))
                    C.embedding_fwd_ids(Wd, ar.put(ids), out, mz)
                    assert ar.ok() and am.same_bits(out.cpu(), am.emb_fwd_oracle(W, ids, mz)), (D, rows, mz, ow, oo)
            if ids_dt == torch.int64:
                idx = ids - 1
                ar = _Arena()
                Wd, out = ar.put(W, 1), ar.new(rows * D, F32, 0, (rows, D))
                C.embedding_fwd(Wd, ar.put(idx), out)
                assert ar.ok() and am.same_bits(out.cpu(), am.emb_fwd_idx_oracle(W, idx)), (D, rows)
    rows, D = am.ROWS_PAST_CAP, 4                              # second trip: more rows than 16384 x 4 waves
    W = torch.randn(nIndex, D, generator=am.gen(1))
    ids = am.emb_ids(rows, nIndex, 5, ids_dt)
    ar = _Arena()
    out = ar.new(rows * D, F32, 0, (rows, D))
    C.embedding_fwd_ids(ar.put(W), ar.put(ids), out, True)
    assert ar.ok() and am.same_bits(out.cpu(), am.emb_fwd_oracle(W, ids, True))


def _emb_bwd_cases():
    nIndex = 11
    for D, rows, gdt, idt in ((1, 5, F32, F32), (5, 9, F32, torch.int64), (64, 33, BF, F32), (65, 70, F32, F32),
                              (130, 40, BF, torch.int64), (4, 4096, F32, F32), (260, 3, F32, torch.int64)):
        ids = am.emb_ids(rows, nIndex, D + rows, idt)
        if rows == 4096:
            ids = torch.full((rows,), 7).to(idt)               # heavy collision: every row on one id
        g = torch.randint(-4, 5, (rows, D), generator=am.gen(D)).to(gdt)
        gW0 = torch.randint(-4, 5, (nIndex, D), generator=am.gen(D + 1)).float()
        yield nIndex, D, rows, ids, g, gW0


@pytest.mark.parametrize("det", [False, True], ids=["atomics", "sorted"])
def test_embedding_backward_exact(det):
    """Integer gradients, dyadic scale: any order gives the same sum. += onto a pre-loaded gW, the padding id skipped,
    rows that no id names untouched by bits; both routes (the binding routes on the deterministic mode)."""
    C = _n()
    with _det(det):
        for nIndex, D, rows, ids, g, gW0 in _emb_bwd_cases():
            for pad in (-1, 2):
                keys = am.emb_keys(ids, pad)
                want, _, run = am.emb_bwd_oracle(gW0, keys, g, 0.5)
                ar = _Arena()
                gW = ar.put(gW0, 1)
                C.embedding_bwd_ids(ar.put(g), ar.put(ids), gW, pad, 0.5)
                assert ar.ok() and am.st.is_f32(want)
                assert torch.equal(gW.cpu().to(F64), want), (D, rows, pad)
                assert am.same_bits(gW.cpu()[run == 0], gW0[run == 0]), (D, rows, pad)
            if g.dtype == F32:
                ar = _Arena()
                gW = ar.put(gW0)
                C.embedding_bwd(ar.put(g), ar.put(ids.long() - 1), gW, 0.5)
                want, _, _ = am.emb_bwd_oracle(gW0, ids.long() - 1, g, 0.5)
                assert ar.ok() and torch.equal(gW.cpu().to(F64), want), (D, rows)


def test_embedding_sorted_route_gaussian_and_bitwise_repeat():
    """Deterministic mode on Gaussian data: per element within 2^-24 (run length + 1) sum |terms|; two launches equal."""
    C = _n()
    with _det(True):
        for D, rows in ((65, 70), (130, 300), (4, 4096)):
            nIndex = 11
            ids = am.emb_ids(rows, nIndex, D, F32) if rows != 4096 else torch.full((rows,), 3.0)
            g = torch.randn(rows, D, generator=am.gen(D))
            gW0 = torch.randn(nIndex, D, generator=am.gen(D + 1))
            keys = am.emb_keys(ids, -1)
            want, mag, run = am.emb_bwd_oracle(gW0, keys, g, 0.3)
            outs = []
            for _ in range(2):
                ar = _Arena()
                gW = ar.put(gW0)
                C.embedding_bwd_ids(ar.put(g), ar.put(ids), gW, -1, 0.3)
                assert ar.ok()
                outs.append(gW.cpu())
            assert am.same_bits(outs[0], outs[1])
            bound = am.U24 * (run[:, None].to(F64) + 1) * mag
            assert _report("emb_det", f"D={D} rows={rows}", am.elem_ratio(outs[0], want, bound)) <= _allowed("emb_det")


# ================================================================================================== resize
def _resize(x, OH, OW, align):
    sh, sw = am.resize_scales(x.shape[2], x.shape[3], OH, OW, align)
    ar = _Arena()
    y = ar.new(x.shape[0] * x.shape[1] * OH * OW, F32, 0, x.shape[:2] + (OH, OW))
    _n().resize_bilinear_fwd(ar.put(x), y, sh, sw)
    assert ar.ok(), ("canary", tuple(x.shape), OH, OW)
    return y


def _resize_bwd(gy, H, W, align):
    sh, sw = am.resize_scales(H, W, gy.shape[2], gy.shape[3], align)
    ar = _Arena()
    gx = ar.new(gy.shape[0] * gy.shape[1] * H * W, F32, 0, gy.shape[:2] + (H, W))
    gx.zero_()
    _n().resize_bilinear_bwd(ar.put(gy), gx, sh, sw)
    assert ar.ok()
    return gx


@pytest.mark.parametrize("align", [False, True], ids=["legacy", "align"])
def test_resize_geometry(align):
    """Every geometry: Gaussian data in ulps of the largest corner; integer data exact where the fractions are dyadic
    (identity, exact 2x, align_corners with a dyadic (in - 1) / (out - 1)); backward exact on integer gy there, and
    within 2^-24 (contributions + 1) sum |terms| on Gaussian data."""
    geos = am.RESIZE_GEO + ((5, 9, 9, 17), (1000, 2, 3000, 3), (2, 1000, 3, 3000))
    for H, W, OH, OW in geos:
        x = torch.randn(2, 3, H, W, generator=am.gen(H + 7 * OW))
        want, mag = am.resize_oracle(x, OH, OW, align)
        r = _report("resize_fwd", f"{H}x{W}->{OH}x{OW}", am.elem_ratio(_resize(x, OH, OW, align).cpu(), want, am.ulp32(mag)))
        assert r <= _allowed("resize_fwd")
        gy = torch.randn(2, 3, OH, OW, generator=am.gen(OH))
        gw, gm, cnt = am.resize_bwd_oracle(gy, H, W, align)
        r = _report("resize_bwd", f"{H}x{W}->{OH}x{OW}",
                    am.elem_ratio(_resize_bwd(gy, H, W, align).cpu(), gw, am.U24 * (cnt + 1) * gm + am.TINY))
        assert r <= _allowed("resize_bwd")
        sh, sw = am.resize_scales(H, W, OH, OW, align)
        if all(float(s * 4).is_integer() for s in (sh, sw)):   # fractions in {0, .25, .5, .75}: exact on integers
            xi = torch.randint(-8, 9, (2, 3, H, W), generator=am.gen(3)).float()
            wi, _ = am.resize_oracle(xi, OH, OW, align)
            assert torch.equal(_resize(xi, OH, OW, align).cpu().to(F64), wi), (H, W, OH, OW)
            gi = torch.randint(-8, 9, (2, 3, OH, OW), generator=am.gen(4)).float()
            gwi, _, _ = am.resize_bwd_oracle(gi, H, W, align)
            assert torch.equal(_resize_bwd(gi, H, W, align).cpu().to(F64), gwi), (H, W, OH, OW)


def test_resize_second_grid_stride_trip():
    """NC = 1, output 2049 x 2049 (past 16384 x 256 elements), align_corners scale 0.5 on integers: exact."""
    x = torch.randint(-8, 9, (1, 1, 1025, 1025), generator=am.gen(1)).float()
    y = _resize(x, 2049, 2049, True)                           # (1025 - 1) / (2049 - 1) = 0.5
    want, _ = am.resize_oracle(x, 2049, 2049, True)
    assert torch.equal(y.cpu().to(F64), want)


# ================================================================================================== log-softmax
def _lsm(x):
    ar = _Arena()
    y = ar.new(x.numel(), F32, 0, x.shape)
    _n().log_softmax_fwd(ar.put(x), y)
    assert ar.ok(), ("canary", tuple(x.shape))
    return y.cpu()


def test_log_softmax_forward_backward():
    for cols in am.LSM_COLS:
        for rows in am.LSM_ROWS:
            for sigma, off in ((1.0, 0.0), (4.0, 0.0), (30.0, 0.0), (1.0, 1e4)):
                x = am.lsm_gauss(rows, cols, sigma, off, cols + rows)
                want = am.lsm_oracle(x)
                y = _lsm(x)
                r = _report("lsm_fwd", f"{rows}x{cols} sigma={sigma} off={off}", am.elem_ratio(y, want, am.lsm_bound(x)))
                assert r <= _allowed("lsm_fwd"), (rows, cols, sigma, off)
                if cols == 1:
                    assert am.same_bits(y, torch.zeros(rows, 1))
            yo = am.lsm_oracle(am.lsm_gauss(rows, cols, 4.0, 0.0, 5)).to(F32)
            gy = torch.randn(rows, cols, generator=am.gen(6))
            ar = _Arena()
            gx = ar.new(rows * cols, F32, 0, (rows, cols))
            _n().log_softmax_bwd(ar.put(yo), ar.put(gy), gx)
            assert ar.ok()
            gw, bound = am.lsm_bwd_oracle(yo, gy)
            assert _report("lsm_bwd", f"{rows}x{cols}", am.elem_ratio(gx.cpu(), gw, bound)) <= _allowed("lsm_bwd")


def test_log_softmax_infinities_and_second_trip():
    for cols in (2, 65, 1000):
        x = am.lsm_gauss(6, cols, 2.0, 0.0, cols)
        x[1] = -float("inf")                                   # a whole row: NaN as in torch, its neighbours untouched
        x[2, 0] = -float("inf")                                # first in lane 0's stride
        x[3, cols - 1] = -float("inf")
        x[4, cols // 2] = float("inf")                         # pinned to torch: the row is NaN
        y = _lsm(x)
        want = am.lsm_oracle(x)
        assert torch.equal(torch.isnan(torch.log_softmax(x, 1)), torch.isnan(want))
        assert am.elem_ratio(y, want, am.lsm_bound(x)) <= _allowed("lsm_fwd"), cols
    rows = am.ROWS_PAST_CAP
    x = am.lsm_gauss(rows, 3, 2.0, 0.0, 1)
    r = _report("lsm_fwd", "65537x3", am.elem_ratio(_lsm(x), am.lsm_oracle(x), am.lsm_bound(x)))
    assert r <= _allowed("lsm_fwd")
    from bigdl_amd.ops import nnk

    x = am.lsm_gauss(5, 65, 2.0, 0.0, 2)
    p = nnk.softmax(x.to(DEV)).cpu()
    assert torch.allclose(p.to(F64), torch.softmax(x.to(F64), 1), rtol=1e-5, atol=1e-30)


# ================================================================================================== modules
@pytest.mark.parametrize("kind", list(am.ACT))
def test_activation_layers_route_to_the_kernels(kind):
    """n = 1003 flat fp32 and channels-last bf16 through the layer: native route taken, the binding legs' bound holds,
    backward too; a strided view with gaps takes the autograd path."""
    from bigdl_amd import nn

    _, a, b = am.ACT[kind]
    args = {"ELU": (a,), "LeakyReLU": (a,), "SoftPlus": (a,), "HardTanh": (a, b), "SoftShrink": (a,), "HardShrink": (a,),
            "Threshold": (a, b)}.get(kind, ())
    m = getattr(nn, kind)(*args)
    for dtype, shape, cl in ((F32, (1003,), False), (BF, (2, 8, 9, 7), True)):
        n = 1003 if not cl else 2 * 8 * 9 * 7
        x = am.act_gauss(kind, n, 21, dtype).view(shape)
        xd = x.to(DEV).contiguous(memory_format=torch.channels_last) if cl else x.to(DEV)
        y = m.forward(xd)
        assert m._native_x is not None and y.stride() == xd.stride()
        want = am.act_f64(kind, x, a, b)
        tag = f"{kind} layer {DT_IDS[DTS.index(dtype)]}"
        assert _report("act_fwd", tag, am.elem_ratio(y.cpu(), want, am.act_bound(kind, x, a, b))) <= \
            _allowed("act_fwd", kind, dtype)
        dy = torch.randn(shape, generator=am.gen(2)).to(dtype)
        dx = m.backward(xd, dy.to(DEV))
        dxw = dy.to(F64) * am.act_df64(kind, x, y.cpu(), a, b)
        assert _report("act_bwd", tag, am.elem_ratio(dx.cpu(), dxw, am.act_dbound(kind, x, y.cpu(), dy, a, b))) <= \
            _allowed("act_bwd", kind, dtype)
    xs = am.act_gauss(kind, 2006, 4, F32).to(DEV)[::2]
    ys = m.forward(xs)
    assert m._native_x is None and ys.shape == xs.shape


def test_misc_layers_agree_with_the_cpu_engine():
    """One case per layer: the GPU layer takes the native route (LookupTable says so itself; the others have no other
    route on a device tensor: ops/nnk.py raises without the extension) and agrees with the CPU engine within the
    binding legs' bounds, taken against the fp64 oracle on both sides."""
    from bigdl_amd import nn

    torch.manual_seed(0)
    lt = nn.LookupTable(11, 6, maskZero=True)
    ids = torch.tensor([[1.0, 11.0, 0.0], [4.0, 4.0, 7.0]])
    want = lt.forward(ids).clone()
    lt.cuda()
    assert lt._native_ids(ids.to(DEV))
    assert torch.equal(lt.forward(ids.to(DEV)).cpu(), want)       # the masked row: +0 here, x * 0 on the CPU engine

    def both(m, x, oracle, bound, allowed):
        w = oracle.to(F64)
        for got in (m.forward(x).clone(), m.forward(x.to(DEV)).cpu()):
            assert am.elem_ratio(got, w, bound) <= allowed, type(m).__name__

    x = torch.randn(2, 7, 5, 6)
    yw, sw = am.lrn_oracle(x, 5, 1.0, 0.75, 1.0)
    both(nn.SpatialCrossMapLRN(5, 1.0, 0.75, 1.0), x, yw, am.lrn_y_bound(yw, sw, 0.75), _allowed("lrn_y"))
    x = torch.randn(2, 3, 5, 7)
    yw, mag = am.resize_oracle(x, 9, 4, False)
    both(nn.ResizeBilinear(9, 4), x, yw, am.ulp32(mag), _allowed("resize_fwd"))
    x = torch.randn(5, 37)
    both(nn.LogSoftMax(), x, am.lsm_oracle(x), am.lsm_bound(x), _allowed("lsm_fwd"))
