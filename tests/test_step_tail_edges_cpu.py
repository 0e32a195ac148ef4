"""tests/step_tail_edge_cases.py on its own: the oracles against torch, the exact data really exact in fp32, the
geometry mirrors at the sizes the GPU file uses, and the sensitivity of every comparison the GPU file makes: a result
that is wrong in one element (one ulp, a shifted target column, a segment boundary off by one, a dropped tail element)
is rejected by the same function that accepts the oracle."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import step_tail_edge_cases as st  # noqa: E402

BF, F32, F64 = st.BF, st.F32, st.F64


def _next_up(t):
    """One ulp up (by bit pattern, away from zero) in t's own format."""
    b = st.bits(t).clone()
    return (b + 1).view(t.dtype)


# ------------------------------------------------------------------------------------------------ geometry
def test_mirrors_reach_the_branches_they_name():
    assert st.grid_cap(1) == 1 and st.grid_cap(8192 * 256) == 8192 and st.grid_cap(8192 * 256 + 1) == 8192
    assert st.SGD4_PAST_CAP % 4 == 0 and st.SGD1_PAST_CAP % 4 == 1 and st.CAST_PAST_CAP % 4 == 1
    assert st.RELU_PAST_CAP % 8 == 3 and st.FILL_PAST_CAP % 16 == 5
    assert st.xent_blocks(st.XENT_PAST_CAP_ROWS) == st.XENT_SLOTS < (st.XENT_PAST_CAP_ROWS + 3) // 4
    assert st.xent_blocks(8192) == 2048 and (8192 + 3) // 4 == 2048      # 8192 rows: still one trip
    assert st.RTZ_PAST_CAP == 16384 * 256 * 4 + 5 and st.grid_cap(st.CAST_PAST_CAP // 4, st.RTZ_CAP) == 8193
    paths = {(K, bf): st.xent_path(K, bf) for K in st.XENT_K for bf in (True, False)}
    assert paths[(7, True)] == ("scalar", 1) and paths[(8, True)] == ("vec", 1) and paths[(8, False)] == ("vec", 1)
    assert paths[(65, False)] == ("scalar", 2) and paths[(72, True)] == ("vec", 1) and paths[(72, False)] == ("vec", 1)
    assert paths[(520, True)] == ("vec", 2) and paths[(512, True)] == ("vec", 1) and paths[(512, False)] == ("vec", 2)
    assert paths[(1000, True)] == ("vec", 2) and paths[(1003, True)] == ("scalar", 16)
    assert {p for p, _ in paths.values()} == {"vec", "scalar"}
    assert st.colsum_past_cap_case() == (2048 * 256 + 1, 8)
    P, K = st.colsum_past_cap_case()
    bx, by, rpb = st.colsum_grid(P, K, False)
    assert bx * by == 2048 and by * rpb >= P and rpb == 257
    P, K = st.COLSUM_DET_PAST_SLOTS
    bx, by, rpb = st.colsum_grid(P, K, True)
    assert (P + 255) // 256 > st.DET_SLOTS and by <= st.DET_SLOTS and by * rpb >= P
    assert st.colsum_grid(257, 24, False) == (1, 2, 129)


# ------------------------------------------------------------------------------------------------ comparisons
def test_ulp_and_bit_comparisons_see_one_ulp():
    v = torch.tensor([1.0, -3.5, 1e-3, 2.0 ** -140, 0.0], dtype=F32)
    assert st.ulp_dist(v, v.double()) == 0.0
    assert st.ulp_dist(_next_up(v)[:4], v[:4].double()) == 1.0
    assert st.same_bits(v, v.clone()) and not st.same_bits(v, _next_up(v))
    assert not st.same_bits(torch.tensor([0.0]), torch.tensor([-0.0]))
    b = torch.tensor([1.0, float("nan"), -2.0]).to(BF)
    assert st.same_bits_nan(b, b.clone()) and not st.same_bits_nan(b, _next_up(b))
    assert not st.same_bits_nan(torch.tensor([1.0, 0.0, -2.0]).to(BF), b)        # a cleaned NaN is seen
    assert st.equals_f64(v, v.double()) and not st.equals_f64(_next_up(v), v.double())
    assert float(st.bf16_half_spacing(torch.tensor([1.0, 1.5, 2.0], dtype=F64))[1]) == 2.0 ** -8
    assert st.is_f32(torch.tensor([0.5, 3.0], dtype=F64)) and not st.is_f32(torch.tensor([0.1], dtype=F64))


def test_canaries_see_a_write_on_either_side():
    for dtype, off in ((F32, 0), (BF, 3), (torch.uint8, 2)):
        v, full, lead = st.guarded(10, dtype, "cpu", off)
        nb = 10 * v.element_size()
        v.zero_()
        assert st.canaries_ok(full, lead, nb) and v.data_ptr() - full.data_ptr() == st.GUARD + off * v.element_size()
        full[lead + nb] = 0
        assert not st.canaries_ok(full, lead, nb)
        full[lead + nb] = st.SENTINEL
        full[lead - 1] = 0
        assert not st.canaries_ok(full, lead, nb)


# ------------------------------------------------------------------------------------------------ softmax + NLL
@pytest.mark.parametrize("K", st.XENT_K)
def test_xent_oracle_is_torch_cross_entropy(K):
    B = 5
    x = st.xent_gauss(B, K, 4.0, 0.0, K, F32)
    labels = torch.randint(1, K + 1, (B,), generator=st.gen(K)).float()
    labels[0], labels[B - 1] = 0.0, K + 1.0                   # both out of range with base 1: skipped rows
    loss, grad, rows, valid = st.xent_oracle(x, labels, 1.0, 0.25)
    assert valid.tolist() == [False] + [True] * (B - 2) + [False]
    xd = x.double().requires_grad_()
    tgt = torch.where(valid, labels.long() - 1, torch.full((B,), -100))
    ref = F.cross_entropy(xd, tgt, reduction="sum", ignore_index=-100) * 0.25
    ref.backward()
    ref = ref.detach()
    assert abs(float(loss) - float(ref)) <= 1e-12 * max(1.0, abs(float(ref)))
    assert torch.allclose(grad, xd.grad, rtol=1e-12, atol=1e-15)
    assert bool((grad[0] == 0).all()) and bool((grad[-1] == 0).all()) and rows[0] == 0 and rows[-1] == 0


def test_xent_exact_legs_are_exact():
    for K in (1, 2, 8, 64, 512, 1024):
        for scale in (1.0, 1.0 / 4, 8.0):
            x = st.xent_uniform(4, K)
            labels = torch.tensor([1.0, K, (K + 1) // 2, 1.0])
            _, grad, _, _ = st.xent_oracle(x, labels, 1.0, scale)
            onehot = F.one_hot(labels.long() - 1, K).double()
            want = st.xent_uniform_expect(K, labels, 1.0, scale)
            assert torch.equal(want, (1.0 / K - onehot) * scale) and st.is_f32(want)
            assert torch.allclose(grad, want, rtol=1e-14, atol=1e-16)
    for K in (7, 8, 65, 520):
        cols, labs = [0, K - 1, K // 2], torch.tensor([1.0, 1.0, K // 2 + 1.0])
        x = st.xent_spike(3, K, cols)
        loss, grad, rows, _ = st.xent_oracle(x, labs, 1.0, 0.5)
        rows_e, want = st.xent_spike_expect(K, cols, labs, 1.0, 0.5)
        assert want[1, K - 1] == 0.5 and want[1, 0] == -0.5 and float(want.abs().sum()) == 1.0
        assert torch.equal(grad.float().double(), want)         # exp(-200) is below fp32, the oracle rounds to it
        assert rows.float().tolist() == rows_e.tolist() == [0.0, 100.0, 0.0] and st.is_f32(want)


def test_xent_comparisons_reject_a_shifted_target_and_one_bf16_ulp():
    B, K = 4, 72
    x = st.xent_gauss(B, K, 4.0, 0.0, 3, BF)
    labels = torch.tensor([1.0, 9.0, 72.0, 33.0])
    _, grad, _, _ = st.xent_oracle(x, labels, 1.0, 1.0)
    for dt in (BF, F32):
        good = grad.to(dt)
        assert st.xent_grad_ratio(good, x, grad, 1.0) <= 1.0
        _, shifted, _, _ = st.xent_oracle(x, labels + 1 - 2 * (labels == K), 1.0, 1.0)
        assert st.xent_grad_ratio(shifted.to(dt), x, grad, 1.0) > 1e3
    bad = grad.to(BF)
    bad[2, 5] = _next_up(bad[2, 5:6])[0]
    assert 1.0 < st.xent_grad_ratio(bad, x, grad, 1.0)          # the allowed bf16 ratio is 1: the bound as derived
    g, gs = (st.xent_uniform_expect(8, torch.tensor(l), 1.0, 1.0) for l in ([3.0, 8.0], [4.0, 8.0]))
    assert st.equals_f64(g.float(), g) and not st.equals_f64(gs.float(), g)
    assert not st.equals_f64(_next_up(g.float()), g)


def test_xent_neg_inf_cases_and_loss_units():
    for K, per in ((7, 8), (72, 8), (520, 8), (1003, 8), (65, 4), (512, 4)):
        cases = st.xent_neg_inf_cases(K, per)
        assert "first_of_lane0" in cases and all(0 < len(c) < K for c in cases.values())
        x = st.xent_gauss(2, K, 1.0, 0.0, K, F32)
        for cols in cases.values():
            y = x.clone()
            y[:, cols] = -float("inf")
            lab = torch.tensor([float([c for c in range(K) if c not in cols][0] + 1)] * 2)
            loss, grad, _, _ = st.xent_oracle(y, lab, 1.0, 1.0)
            assert torch.isfinite(loss) and bool((grad[:, cols] == 0).all()) and bool(torch.isfinite(grad).all())
    loss, grad, _, _ = st.xent_oracle(torch.full((1, 8), -float("inf")), torch.tensor([1.0]), 1.0, 1.0)
    assert torch.isnan(loss) and bool(torch.isnan(grad).all())            # torch: an all -inf row is NaN
    x = st.xent_gauss(5, 64, 4.0, 80.0, 1, F32)
    reorder, unit = st.xent_loss_units(x, torch.arange(1, 6).float(), 1.0, 1.0, st.xent_blocks(5))
    assert reorder > 0 and unit > 5 * st.U24 * 160


# ------------------------------------------------------------------------------------------------ SGD
@pytest.mark.parametrize("hp", st.SGD_EXACT_HP)
def test_sgd_exact_data_is_exact_and_the_oracle_is_the_cpu_engine(hp):
    from bigdl_amd.optim.sgd import SGD

    lr, wd, momentum, dampening, nesterov = hp
    for n in st.SGD_N:
        w0, steps, exact = st.sgd_exact_run(n, hp, n)
        assert exact, (hp, n)
        opt = SGD(learningRate=lr, weightDecay=wd, momentum=momentum, dampening=dampening, nesterov=nesterov)
        w = w0.clone()
        for g, w_after, mom_after in steps:
            opt.optimize(lambda _w, _g=g: (0.0, _g), w)
            assert st.equals_f64(w, w_after), (hp, n)
            if momentum:
                assert st.equals_f64(opt.state["dfdx"], mom_after)
            assert st.is_f32(w_after) and torch.equal(w.to(BF), w_after.float().to(BF))


@pytest.mark.parametrize("name", sorted(st.seg_cases()))
def test_segment_oracle_is_the_fallback_and_sees_a_moved_boundary(name):
    from bigdl_amd.optim.sgd import segment_decay_vector

    off, wd, base, n = st.seg_cases()[name]
    assert all(st.is_f32(torch.tensor([v], dtype=F64)) for v in wd) and off[0] <= base
    dec = st.seg_decay_vector(off, wd, n, base)
    seg = (torch.tensor(off, dtype=torch.int64), torch.tensor(wd, dtype=F32))
    assert torch.equal(segment_decay_vector(seg, n, base, "cpu").double(), dec), name
    hp = (0.5, 0.125, 0.75, 0.5, False)
    _, steps, exact = st.sgd_exact_run(n, hp, 5, decay=dec)
    assert exact, name
    if len(off) > 1:
        i = max(k for k in range(1, len(off)) if base < off[k] < base + n or k == 1)
        if base < off[i] < base + n and wd[i] != wd[i - 1]:
            moved = list(off)
            moved[i] += 1
            _, other, _ = st.sgd_exact_run(n, hp, 5, decay=st.seg_decay_vector(moved, wd, n, base))
            assert not st.equals_f64(other[-1][1].float(), steps[-1][1]), name


def test_segment_below_the_first_offset_takes_segment_zero_on_both_routes():
    """The kernels' seg_decay gives an element below seg_off[0] segment 0's decay.
    fold_regularizers starts the first segment at 0, so a training step has no such element; the fallback agrees."""
    from bigdl_amd.optim.sgd import segment_decay_vector

    seg = (torch.tensor([6, 10]), torch.tensor([0.5, 0.25]))
    want = st.seg_decay_vector([6, 10], [0.5, 0.25], 12, 2)
    assert want.tolist() == [0.5] * 8 + [0.25] * 4
    assert torch.equal(segment_decay_vector(seg, 12, 2, "cpu").double(), want)


def test_sgd_comparison_rejects_a_dropped_tail_element_and_one_ulp():
    hp = st.SGD_EXACT_HP[0]
    w0, steps, _ = st.sgd_exact_run(1027, hp, 1)
    _, w1, m1 = steps[0]
    got = w1.float()
    assert st.equals_f64(got, w1) and st.same_bits(got.to(BF), w1.float().to(BF))
    dropped = got.clone()
    dropped[-1] = w0[-1]                                      # the scalar tail element not updated
    assert not st.equals_f64(dropped, w1)
    assert not st.equals_f64(_next_up(got), w1)
    assert not st.same_bits(_next_up(got.to(BF)), w1.float().to(BF))


# ------------------------------------------------------------------------------------------------ Adam / adaptive
def test_adam_oracle_is_the_cpu_engine():
    from bigdl_amd.optim.methods import Adam

    for wd, eps in ((0.0, 1e-8), (1e-2, 1e-3)):
        n = 1027
        w = torch.randn(n, generator=st.gen(1))
        opt = Adam(1e-3, 0.0, 0.9, 0.999, eps, wd)
        m = v = torch.zeros(n)
        for t in (1, 2, 3):
            g = torch.randn(n, generator=st.gen(10 + t))
            g[::7] = 0.0
            we, me, ve, mag = st.adam_oracle(w, g, m, v, 1e-3, 0.9, 0.999, eps, wd, t)
            opt.optimize(lambda _w, _g=g: (0.0, _g), w)
            assert st.ulp_dist(w, we, mag=mag["w"]) <= 4 and st.ulp_dist(opt.state["s"], me, mag=mag["m"]) <= 4
            assert st.ulp_dist(opt.state["r"], ve, mag=mag["v"]) <= 4
            m, v = opt.state["s"].clone(), opt.state["r"].clone()
        assert bool(torch.isfinite(w).all())
    z = torch.zeros(2)
    we, me, ve, _ = st.adam_oracle(torch.ones(2), z, z, z, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1)
    assert we.tolist() == [1.0, 1.0] and me.tolist() == [0.0, 0.0]           # 0 / (0 + eps)


@pytest.mark.parametrize("mid,name,hp,two,s1_0", st.OPTIM_METHODS, ids=[m[1] for m in st.OPTIM_METHODS])
def test_optim_oracle_is_the_cpu_engine(mid, name, hp, two, s1_0):
    from bigdl_amd.optim import methods as M

    make = {"adagrad": lambda: M.Adagrad(0.1, 0.0, 1e-3), "rmsprop": lambda: M.RMSprop(0.01, 0.0, 0.9, 1e-6),
            "adadelta": lambda: M.Adadelta(0.9, 1e-6), "adamax": lambda: M.Adamax(0.02, 0.9, 0.999, 1e-38),
            "ftrl": lambda: M.Ftrl(0.1, -0.5, 0.1, 0.01, 0.02, 0.03),
            "ftrl_pow": lambda: M.Ftrl(0.1, -0.6, 0.1, 0.01, 0.02, 0.0)}[name]
    n = 1027
    x = torch.randn(n, generator=st.gen(2))
    g = torch.randn(n, generator=st.gen(3))
    s1 = torch.full((n,), s1_0)
    s2 = torch.zeros(n) if two else None
    xe, s1e, s2e, mag = st.optim_oracle(mid, hp, x, g, s1, s2)
    opt = make()
    opt.optimize(lambda _w: (0.0, g), x)                        # first step: the adamax rate is lr / (1 - b1)
    assert torch.allclose(x.double(), xe, rtol=2e-5, atol=1e-6), name
    assert st.ulp_dist(x, xe, mag=mag.get("x")) <= (64 if name == "ftrl_pow" else 8), name
    assert bool(torch.isfinite(xe).all()) and bool(torch.isfinite(s1e).all())
    assert not torch.allclose(x.double()[:-1], xe[1:], rtol=2e-5, atol=1e-6)     # and it is not a trivial match


# ------------------------------------------------------------------------------------------------ sumsq / colsum
def test_integer_sums_stay_exact_in_fp32():
    for n in st.SUMSQ_N + (st.SUMSQ_PAST_CAP,):
        assert n * 16 + 1024 < 2 ** 24                          # |x| <= 4, any order of adding, + the start value
        x = st.int_vec(n, n, 4)
        assert st.sumsq_oracle(x, 1024.0) == float((x * x).sum()) + 1024.0
        assert st.sumsq_chain(n, "default") >= 12 and st.sumsq_chain(n, "det_ws") == (n + 32767) // 32768 + 139
    for P in st.COLSUM_P + (st.COLSUM_DET_PAST_SLOTS[0], st.colsum_past_cap_case()[0]):
        assert P * 4 + 64 < 2 ** 24
    x = st.int_rows_bf16(257, 24, 1)
    start = torch.arange(24).float()
    want = st.colsum_oracle(x, start)
    assert st.is_f32(want) and torch.equal(want, x.float().sum(0).double() + start.double())
    assert int(x.float().abs().max()) == 4
    assert st.equals_f64(want.float(), want)
    assert bool(x[256].any()) and bool(x[:, 23].any())
    assert not st.equals_f64(want.float() - x[256].float(), want)            # the last row dropped
    k = int(x[256].float().abs().argmax())
    bad = want.float()
    bad[k] -= float(x[256, k])                                  # the last row dropped in one column only
    assert float(x[256, k]) != 0 and not st.equals_f64(bad, want)
    bad = want.float()
    bad[k] = st.bits(bad[k:k + 1]).add(1).view(torch.float32)[0]             # one fp32 ulp in one column
    assert not st.equals_f64(bad, want)
    g = torch.randn(1000, generator=st.gen(0))
    assert abs(float((g * g).sum()) - st.sumsq_oracle(g)) <= st.sumsq_bound(g, 0.0, "default")


# ------------------------------------------------------------------------------------------------ casts
def test_cast_oracles_at_the_rounding_edges():
    tab = st.cast_edge_bits()
    x = tab.view(F32)
    rne, rtz = st.bits(st.rne_oracle(x)).int() & 0xFFFF, st.bits(st.rtz_oracle(x)).int() & 0xFFFF
    at = {int(b) & 0xFFFFFFFF: (int(r), int(z)) for b, r, z in zip(tab, rne, rtz)}
    assert at[0x3F808000] == (0x3F80, 0x3F80) and at[0x3F818000] == (0x3F82, 0x3F81)      # ties to even
    assert at[0x3F807FFF][0] == 0x3F80 and at[0x3F808001][0] == 0x3F81
    assert at[0x3F817FFF][0] == 0x3F81 and at[0x3F818001][0] == 0x3F82
    assert at[0x7F7FFFFF] == (0x7F80, 0x7F7F) and at[0xFF7FFFFF] == (0xFF80, 0xFF7F)      # inf / largest bf16
    assert at[0x7F7F7FFF][0] == 0x7F7F and at[0x7F7F8000][0] == 0x7F80
    assert at[0x00008000] == (0x0000, 0x0000) and at[0x00008001] == (0x0001, 0x0000)      # denormals round too
    assert at[0x80000000] == (0x8000, 0x8000) and at[0x7F800000] == (0x7F80, 0x7F80)
    nan = torch.isnan(x)
    assert int(nan.sum()) == 10 and bool(torch.isnan(st.rne_oracle(x))[nan].all())
    # truncation: a NaN whose payload lies only in the low 16 bits becomes an infinity, any other stays a NaN
    assert at[0x7F800001][1] == 0x7F80 and at[0x7F80FFFF][1] == 0x7F80 and at[0xFF800001][1] == 0xFF80
    assert at[0x7FC00000][1] == 0x7FC0 and at[0x7F810000][1] == 0x7F81
    from bigdl_amd.ops.nnk import f32_to_bf16_rtz

    assert st.same_bits(f32_to_bf16_rtz(x), st.rtz_oracle(x))
    assert not st.same_bits(st.rne_oracle(x), st.rtz_oracle(x))


def test_cast_input_carries_the_table_in_every_residue_and_the_tail():
    tab = st.cast_edge_bits()
    for n in (1003, 2 * 1024 + 5):
        xb = st.bits(st.cast_input(n, 0))
        starts = [i for i in range(n - tab.numel() + 1) if torch.equal(xb[i:i + tab.numel()], tab)]
        assert {s % 4 for s in starts} == {0, 1, 2, 3} and starts[-1] == n - tab.numel()
        assert n - (n // 4) * 4 >= 1                            # the scalar tail holds table entries
    for n in (1, 2, 3, 4, 5):
        assert st.cast_input(n, 0).numel() == n
    good = st.rne_oracle(st.cast_input(1003, 0))
    assert st.same_bits_nan(good, good.clone())
    bad = good.clone()
    bad[-1] = _next_up(bad[-1:])[0] if not torch.isnan(bad[-1]) else 0.0
    assert not st.same_bits_nan(bad, good)


# ------------------------------------------------------------------------------------------------ relu / add
def test_relu_and_add_oracles_against_torch():
    for n in st.RELU_N:
        x, y, dy = st.bf16_input(n, n), st.bf16_input(n, n + 50), st.bf16_input(n, n + 99)
        r = st.relu_fwd_oracle(x)
        t = torch.relu(x.float()).to(BF)
        assert torch.equal(torch.isnan(r), torch.isnan(x)) and torch.equal(torch.isnan(t), torch.isnan(x))
        assert torch.equal(r[~torch.isnan(x)].float(), t[~torch.isnan(x)].float())
        assert not bool((st.bits(r)[(x.float() <= 0)] != 0).any())             # +0, never -0
        b = st.relu_bwd_oracle(dy, y)
        yy = y.float().requires_grad_()
        torch.relu(yy).backward(dy.float())
        ok = ~torch.isnan(y) & ~torch.isnan(dy)
        assert torch.equal(b[ok].float(), yy.grad[ok])
        assert bool(torch.isnan(b[(y.float() > 0) & torch.isnan(dy)]).all())
        assert not bool(st.bits(b)[~(y.float() > 0)].any())
        a = st.add_oracle(x, y)
        assert st.same_bits_nan(a, (x.double() + y.double()).to(BF))       # one rounding of the sum
    x = st.bf16_input(1001, 1)
    assert int(torch.isnan(x).sum()) >= 2
    good = st.relu_fwd_oracle(x)
    cleaned = torch.where(torch.isnan(x), torch.zeros_like(x), good)            # fmaxf(x, 0) semantics
    assert st.same_bits(good, good.clone()) and not st.same_bits(cleaned, good)
    short = good.clone()
    short[-1] = x[-1] if not st.same_bits(x[-1:], good[-1:]) else _next_up(good[-1:])[0]
    assert not st.same_bits(short, good)
