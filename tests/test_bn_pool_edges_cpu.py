"""tests/bn_pool_edge_cases.py checked on its own (no GPU): the exact leg really is exact, the mask sources hold the
values they claim, the pooling oracle agrees with torch where torch's rule is defined, and the bounds of
tests/test_bn_pool_edges_gpu.py would notice a dropped row, a wrong divisor or a truncated output."""
import pytest
import torch
import torch.nn.functional as F

from tests import bn_pool_edge_cases as bp

BF = torch.bfloat16


@pytest.mark.parametrize("C", bp.BN_CHANNELS)
def test_row_counts_reach_every_edge(C):
    rpi, ps = bp.rpi_of(C), bp.row_counts(C)
    assert 1 in ps and rpi in ps and rpi + 1 in ps and (rpi == 1 or rpi - 1 in ps)
    assert any(p % (bp.UNROLL * rpi) not in (0, 1) and p > bp.UNROLL * rpi for p in ps)     # an unrolled tail
    assert any(p > 8 * rpi and p % (8 * rpi) == 1 for p in ps)      # one past whole apply blocks
    # the reduction re-balances its rows per block (ceil(P / blocks)), so its last block is never one row long: the
    # nearest edge is several blocks with a shorter last one
    assert any(bp.reduce_geometry(p, C)[0] > 1 and p % bp.reduce_geometry(p, C)[1] != 0 for p in ps)
    assert not any(bp.reduce_geometry(p, C)[2] or bp.stationary_geometry(p, C)[3] for p in ps)


def test_block_cap_cases_take_the_capped_branch():
    C, P = bp.REDUCE_CAP
    blocks, rpb, capped = bp.reduce_geometry(P, C)
    assert capped and blocks <= 2048 and (blocks - 1) * rpb < P <= blocks * rpb
    C, P = bp.APPLY_CAP
    bx, gy, rpb, capped = bp.stationary_geometry(P, C)
    assert capped and gy == 2 and bx == 4096 and P <= bx * rpb and rpb > 8 * bp.rpi_of(C)
    assert (bx - 1) * rpb >= P              # and the last blocks start past the last row: they must do nothing
    C, P = bp.DET_CAP
    assert not bp.reduce_geometry(P, C)[2] and bp.reduce_geometry(P, C, det=True)[2]
    assert bp.reduce_geometry(P, C, det=True)[0] <= 2 * bp.STAT_SLOTS
    N, C, H, W = bp.MAXPOOL_BIG[1]
    assert N * (H // 2) * (W // 2) * (C // 8) > 8192 * 256
    N, C, H, W = bp.BNRED_BIG
    assert N * (H // 2) * (W // 2) * (C // 8) > 2048 * 256 and 256 % (C // 8) == 0


@pytest.mark.parametrize("C", bp.BN_CHANNELS)
def test_integer_sums_stay_exact_in_fp32(C):
    """Sum of |terms| per channel below 2^23 (terms are multiples of 0.5), from the data alone; and an fp32 sum in
    another order lands on the fp64 value."""
    for P in bp.row_counts(C):
        x, dz, mean = bp.stats_inputs(P, C), bp.int_rows(P, C, 2, bp.DMAX), bp.half_means(C, 1)
        assert x.abs().max() <= bp.XMAX and dz.abs().max() <= bp.DMAX and mean.abs().max() <= bp.MEANMAX
        assert torch.equal(mean * 2, (mean * 2).round())
        assert bp.abs_budget(dz, x, mean) < bp.EXACT_LIMIT
        s1, s2 = bp.stats_oracle(x)
        assert torch.equal(x.float().flip(0).sum(0).double(), s1)
        assert torch.equal((x.float() ** 2).sum(0).double(), s2)
        # the marked tail rows: dropping the last row changes both sums in every channel
        assert (x[P - 1].float() >= 3).all()


def test_cap_case_budgets_from_the_ranges():
    """The large cases are generated on the device; their budget follows from the value ranges: P max|dz| (max|x| +
    max|mean|) and P max|x|^2."""
    for C, P in (bp.REDUCE_CAP, bp.APPLY_CAP, bp.DET_CAP):
        assert P * bp.DMAX * (bp.XMAX + bp.MEANMAX) < bp.EXACT_LIMIT and 16 * P < 2 ** 24
    # fused pool backward: sum |dx| <= sum |dy| (every dy lands on one pixel), |dy| <= 2, |x - mean| <= 2 + 2
    N, C, H, W = bp.BNRED_BIG
    assert N * (H // 2) * (W // 2) * 2 * (2 + bp.MEANMAX) < bp.EXACT_LIMIT


def test_mask_sources_hold_the_edge_values():
    P, C = 259, 24
    x = bp.int_rows(P, C, 1)
    z, _, _, m = bp.mask_inputs("z", P, C, x)
    zf = z.float()
    assert (zf == 0).any() and torch.signbit(zf[zf == 0]).any() and (~torch.signbit(zf[zf == 0])).any()
    assert (zf < 0).any() and (zf == 2.0 ** -126).any() and torch.equal(m, zf > 0)
    _, zm, aff, m = bp.mask_inputs("zm+aff", P, C, x)
    assert sorted(set(zm.tolist())) == list(range(256)) and aff is not None
    assert torch.equal(bp.pack_mask(m), zm) and torch.equal(bp.unpack_mask(zm, P, C), m)
    assert m[0, :8].tolist() == [bool((11 >> e) & 1) for e in range(8)]      # bit e of byte 0 is channel e of row 0
    # zm wins over aff: the two masks differ, so a kernel that took aff would be seen
    assert not torch.equal(m, bp.aff_pre(x, aff) > 0)
    _, _, aff, m = bp.mask_inputs("aff", P, C, x)
    pre = bp.aff_pre(x, aff)
    assert (pre[:, 0] == 0).any() and not m[:, 0][pre[:, 0] == 0].any()               # exactly 0: masked
    assert (pre[:, 1] == 2.0 ** -23).any() and m[:, 1][pre[:, 1] == 2.0 ** -23].all()  # smallest positive: kept
    # an unfused fp32 product + add gives 0 there: the case separates the two forms
    xf, a = x.float(), aff
    unfused = (xf[:, 1] * a[1]) + a[C + 1]
    assert (unfused[pre[:, 1] == 2.0 ** -23] == 0).all()
    # every other channel: bf16-representable coefficients, so the fp64 value is an fp32 number
    assert torch.equal(pre[:, 2:].float().double(), pre[:, 2:])


@pytest.mark.parametrize("P,C", [(1, 8), (259, 24), (32769, 1032)])
def test_exact_coefficients_are_fp32_numbers(P, C):
    invstd, gamma, mean, red = bp.exact_coef_inputs(C, P, 1)
    assert torch.equal(red.double(), (red.double() / P * 64).round() * P / 64)
    co = bp.coeff_ref(red, 1, mean, invstd, gamma, P, True)
    for k in ("A", "B", "D"):
        assert torch.equal(co[k].float().double(), co[k]), k
    assert co["B"].abs().max() > 0 and co["D"].abs().max() > 0


def test_finalize_reference_matches_batch_norm():
    P, C = 37, 16
    x = bp.gauss_rows(P, C, 1, 0.5, 2.0).double()
    stats = torch.stack([x.sum(0), (x * x).sum(0)]).view(1, 2, C)
    g, b = torch.randn(C, dtype=torch.float64), torch.randn(C, dtype=torch.float64)
    rm, rv = torch.randn(C, dtype=torch.float64), torch.rand(C, dtype=torch.float64) + 0.5
    ref = bp.finalize_ref(stats, 1, g, b, rm, rv, P, 1e-3, 0.1, True)
    rm2, rv2 = rm.clone(), rv.clone()
    y = F.batch_norm(x, rm2, rv2, g, b, True, 0.1, 1e-3)
    assert torch.allclose(ref["running_mean"], rm2, rtol=1e-12, atol=1e-13)
    assert torch.allclose(ref["running_var"], rv2, rtol=1e-11, atol=1e-13)
    assert torch.allclose(x * ref["scale"] + ref["shift"], y, rtol=1e-10, atol=1e-11)
    ev = bp.finalize_ref(None, 0, g, b, rm, rv, P, 1e-3, 0.1, False)
    assert torch.allclose(x * ev["scale"] + ev["shift"], F.batch_norm(x, rm, rv, g, b, False, 0.1, 1e-3), atol=1e-11)
    # backward coefficients against autograd
    dz = torch.randn(P, C, dtype=torch.float64)
    xs = x.clone().requires_grad_(True)
    F.batch_norm(xs, None, None, g, b, True, 0.1, 1e-3).backward(dz)
    mean, invstd = ref["save_mean"], ref["save_invstd"]
    red = torch.stack(bp.bwd_reduce_oracle(dz, x, mean, torch.ones(P, C, dtype=torch.bool))).view(1, 2, C)
    co = bp.coeff_ref(red, 1, mean, invstd, g, P, True)
    assert torch.allclose(co["A"] * dz + co["B"] * x + co["D"], xs.grad, rtol=1e-9, atol=1e-11)


def test_negative_raw_variance_case_clamps():
    s = torch.tensor([[[3.0], [2.9999998]]])                       # P = 3, mean 1, s2 / P - 1 < 0
    ref = bp.finalize_ref(s, 1, None, None, None, None, 3, 1e-5, 0.1, True)
    assert ref["var_raw"].item() < 0 and ref["save_invstd"].item() == pytest.approx(1e-5 ** -0.5)


def test_ulps_and_bound_notice_small_slips():
    v = torch.tensor([1.0, 3.0, -0.75], dtype=torch.float64)
    assert bp.ulps(v.float() + torch.tensor([2.0 ** -23, 0, 0]), v) == 1.0
    y = bp.gauss_rows(4096, 8, 2).double() * 1.37 + 0.11
    terms = y.abs() + 0.11
    assert ((y.to(BF).double() - y).abs() <= bp.apply_bound(y, terms)).all()           # correct rounding passes
    trunc = (y.float().view(torch.int32) & ~0xffff).view(torch.float32).double()         # truncation does not
    assert not ((trunc - y).abs() <= bp.apply_bound(y, terms)).all()


@pytest.mark.parametrize("P,C", bp.APPLY_SHAPES)
@pytest.mark.parametrize("mode", bp.APPLY_MODES)
def test_apply_inputs_leave_few_undecided_signs(P, C, mode):
    """Where |pre-ReLU| is below the fp32 term the sign mask is not checked: under 0.1 % of the elements."""
    d = bp.apply_inputs(P, C, mode)
    y, pre, terms, extra, pre_m = bp.bn_apply_ref(d["x"], d["scale"], d["shift"], d["res"], d["res_scale"],
                                                  d["res_shift"], d["relu"])
    und = pre_m.abs() < bp.fp32_term(terms)
    if extra is not None:
        assert ((pre_m - pre).abs() <= (0.5 + 2.0 ** -15) * extra).all()     # one bf16 rounding after an fp32 one
    assert und.double().mean().item() < 1e-3
    assert (y >= 0).all() if d["relu"] else (y < 0).any()


# ------------------------------------------------------------------ pooling
def _flat_to_tap(ind, H, W, OH, OW, k, s, p):
    """torch's flat input index -> row-major tap of the window."""
    ih, iw = ind // W, ind % W
    oh = torch.arange(OH).view(1, 1, OH, 1)
    ow = torch.arange(OW).view(1, 1, 1, OW)
    return ((ih - (oh * s - p)) * k + (iw - (ow * s - p))).to(torch.uint8)


@pytest.mark.parametrize("case", bp.MAXPOOL_CASES, ids=lambda c: c[0])
def test_maxpool_oracle_matches_torch_on_ties(case):
    name, shape, k, s, p, ceil = case
    x = bp.int_image(*shape, 1).float().contiguous()
    N, C, H, W = shape
    yt, it = F.max_pool2d(x, k, s, p, ceil_mode=ceil, return_indices=True)
    y, idx = bp.maxpool_oracle(x, k, s, p, ceil)
    assert y.shape == yt.shape and torch.equal(y, yt)
    assert torch.equal(idx, _flat_to_tap(it, H, W, y.shape[2], y.shape[3], k, s, p))
    dy = torch.randint(-4, 5, y.shape).double()
    xs = x.double().requires_grad_(True)
    F.max_pool2d(xs, k, s, p, ceil_mode=ceil).backward(dy)
    assert torch.equal(bp.maxpool_bwd_oracle(dy, idx, H, W, k, s, p), xs.grad)


def test_every_k3_tap_wins_somewhere():
    won = set()
    for name, shape, k, s, p, ceil in bp.MAXPOOL_CASES:
        if k == 3:
            won |= set(bp.maxpool_oracle(bp.int_image(*shape, 1).float(), k, s, p, ceil)[1].unique().tolist())
    assert won == set(range(9))
    # and in the k3 s2 p1 even-size cases alone (the output-centric backward's nine tap tests)
    won = set()
    for name, shape, k, s, p, ceil in bp.MAXPOOL_CASES:
        if (k, s, p) == (3, 2, 1) and shape[2] % 2 == 0 and shape[3] % 2 == 0 and not ceil:
            won |= set(bp.maxpool_oracle(bp.int_image(*shape, 1).float(), k, s, p, ceil)[1].unique().tolist())
    assert won == set(range(9))


def test_all_minus_inf_window_gives_its_gradient_to_the_first_in_bounds_pixel():
    """torch's rule for a window of -inf only, which the oracle follows: 4 x 4 image, k3 s2 p1, the gradient lands on
    (0, 0), (0, 1), (1, 0), (1, 1)."""
    x = torch.full((1, 1, 4, 4), float("-inf"), dtype=torch.float64)
    y, idx = bp.maxpool_oracle(x, 3, 2, 1)
    assert torch.isinf(y).all() and idx.view(-1).tolist() == [4, 3, 1, 0]
    xs = x.clone().requires_grad_(True)
    dy = torch.tensor([[[[1.0, 2.0], [3.0, 5.0]]]], dtype=torch.float64)
    F.max_pool2d(xs, 3, 2, 1).backward(dy)
    dx = bp.maxpool_bwd_oracle(dy, idx, 4, 4, 3, 2, 1)
    assert torch.equal(dx, xs.grad) and dx[0, 0, :2, :2].reshape(-1).tolist() == [1.0, 2.0, 3.0, 5.0]


def test_nan_wins_and_the_last_nan_is_stored():
    x = torch.zeros(1, 1, 3, 3)
    x[0, 0, 0, 1], x[0, 0, 2, 0], x[0, 0, 2, 2] = float("nan"), float("nan"), 9.0
    y, idx = bp.maxpool_oracle(x, 3, 1, 0)
    assert y.isnan().all() and idx.item() == 6


def test_pre_elements_round_once():
    x = bp.int_image(2, 8, 5, 6, 3)
    pre = torch.cat([torch.tensor([0.5, 1.0, -1.0, 1.3, 0.7, 2.0, -0.3, 1.1]).to(BF).float(),
                     torch.tensor([0.0, -1.0, 0.5, 0.2, -0.4, 1.0, 0.3, -2.0]).to(BF).float()])
    v = bp.pre_elements(x, pre)
    want = torch.relu(x.float() * pre[:8].view(1, 8, 1, 1) + pre[8:].view(1, 8, 1, 1)).to(BF)
    assert torch.equal(v, want) and (v.float() != torch.relu(x.float() * pre[:8].view(1, 8, 1, 1) + pre[8:].view(1, 8, 1, 1))).any()


@pytest.mark.parametrize("case", bp.AVGPOOL_CASES, ids=lambda c: c[0])
def test_avgpool_bound_notices_the_wrong_divisor(case):
    name, shape, k, s, p, ceil = case
    x = bp.gauss_rows(shape[0] * shape[2] * shape[3], shape[1], 5).view(shape[0], shape[2], shape[3], shape[1]).permute(0, 3, 1, 2)
    y0 = F.avg_pool2d(x.double(), k, s, p, ceil_mode=ceil, count_include_pad=False)
    dy = torch.ones_like(y0)
    for cp in (True, False):
        y, dx, ya, dxa = bp.avgpool_ref(x, dy, k, s, p, ceil, cp)
        assert ((y.to(BF).double() - y).abs() <= bp.apply_bound(y, ya)).all()
    if p > 0:
        y1 = bp.avgpool_ref(x, dy, k, s, p, ceil, True)[0]
        assert not ((y1 - y0).abs() <= bp.apply_bound(y0, ya)).all()      # count_pad ignored would be seen
