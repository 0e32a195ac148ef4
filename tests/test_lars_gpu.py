"""Fused LARS on the GPU (csrc/lars.hip, bigdl_amd/ops/lars.py) against the oracles of tests/lars_cases.py: the norm
kernels and the update kernel each through their own binding, a two-rank emulation, the route through TrainStep
(plain, mixed with SGD, expanded from one inherited method) and the stand-alone ``LarsSGD.optimize``.

* every tensor a kernel touches is a guarded view inside sentinel bytes; the canaries are checked after the launches;
* the op calls run under torch.cuda.set_sync_debug_mode("error"): nothing in them may wait on the host;
* exact legs are held to equality; Gaussian legs to ``ALLOWED``: 2 x the largest figure measured on an MI355X,
  rounded up, under the leg's cap (profiles/lars_fused_errors.txt holds every measured figure).
"""
import contextlib

import pytest
import torch

from bigdl_amd.ops import lars
from tests import lars_cases as lc
from tests import step_tail_edge_cases as st

pytestmark = pytest.mark.gpu

BF, F32, F64 = st.BF, st.F32, st.F64
DEV = "cuda"
C = lc.CHUNK

# norm: err / worst-case chain bound (cap 1). update_w / update_v: fp32 ulps at the term magnitudes against the fp64
# oracle fed the same fp32 acc (cap 8: the cap of the Adam legs, which also divide and take a root).
CAPS = {"norm": 1.0, "update_w": 8.0, "update_v": 8.0}
ALLOWED = {"norm": 0.08, "update_w": 3.1, "update_v": 4.8}
assert all(ALLOWED[k] <= CAPS[k] for k in CAPS)
SGD_W_ALLOWED = 4.0          # ALLOWED["sgd_w"] of tests/test_step_tail_edges_gpu.py: the SGD pieces of the mixed plan


def _report(name, case, value):
    """One line per measured figure (pytest -s shows them; profiles/lars_fused_errors.txt holds their maxima)."""
    print(f"LARS|{name}|{case}|{value:.4g}")
    return value


def _n():
    from bigdl_amd.ops import native

    Cn = native.get()
    assert (Cn.LARS_CHUNK, Cn.LARS_BLOCK_CAP) == (lc.CHUNK, lc.BLOCK_CAP) == (lars.CHUNK, lars.BLOCK_CAP)
    return Cn


@contextlib.contextmanager
def no_sync():
    torch.cuda.set_sync_debug_mode("error")
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode("default")


@contextlib.contextmanager
def switch(on):
    lars.set_fused(on)
    try:
        yield
    finally:
        lars.set_fused(None)


class _Arena:
    def __init__(self):
        self.items = []

    def new(self, n, dtype, off=0):
        v, full, lead = st.guarded(n, dtype, DEV, off)
        assert full.data_ptr() % 256 == 0
        self.items.append((full, lead, n * v.element_size()))
        return v

    def put(self, src, off=0):
        v = self.new(src.numel(), src.dtype, off)
        v.copy_(src.reshape(-1))
        return v

    def ok(self):
        torch.cuda.synchronize()
        return all(st.canaries_ok(*it) for it in self.items)


class _Bufs:
    """The tables of ``pieces`` on the device and guarded w, g, v, w16, ws, acc, all ``off`` elements past a 16-byte
    boundary (w16: the same element phase). The momentum buffer has the plan's own layout (piece k at lo + dv)."""

    def __init__(self, ar, pieces, nlayers, n, off=0):
        self.pieces, self.nlayers, self.n, self.off = pieces, nlayers, n, off
        self.tab = lars.build_tables(pieces, nlayers)
        self.dev = lars.device_tables(self.tab, DEV)
        self.nchunks = len(self.tab["chunk_piece"])
        self.ws = ar.new(2 * self.nchunks, F32)
        self.acc = ar.new(2 * nlayers, F32)
        self.v = ar.new(self.tab["v_need"], F32, off)
        self.ar = ar

    def put_v(self, v_flat):
        for lo, hi, dv, _ in self.tab["piece_tab"]:
            self.v[lo + dv:hi + dv].copy_(v_flat[lo:hi])

    def get_v(self, like):
        out = like.clone()
        for lo, hi, dv, _ in self.tab["piece_tab"]:
            out[lo:hi] = self.v[lo + dv:hi + dv].cpu()
        return out

    def norms(self, w, g, acc=None):
        d = self.dev
        with no_sync():
            _n().lars_norms(w, g, d["chunk_piece"], d["chunk_start"], d["piece_tab"], d["layer_chunks"], self.ws,
                            self.acc if acc is None else acc, self.tab["max_hi"])
        return self.acc if acc is None else acc

    def update(self, w, g, w16, hp, rate_num, acc, WD):
        d = self.dev
        hp_t = torch.tensor([x for p in hp for x in p], dtype=F32, device=DEV)
        rates = torch.tensor(rate_num, dtype=F32, device=DEV)
        with no_sync():
            _n().lars_update(w, g, self.v, w16, d["chunk_piece"], d["chunk_start"], d["piece_tab"], hp_t, rates, acc,
                             float(WD), self.tab["max_hi"], self.tab["v_need"], self.nlayers)


def _acc32(acc64):
    return acc64.to(F32).to(DEV)


def _hp32(hp):
    return [(lc.f32(a), lc.f32(b)) for a, b in hp]


def _f32s(xs):
    return [lc.f32(x) for x in xs]


# ================================================================================================== norms
@pytest.mark.parametrize("off", (0, 1, 2, 3))
def test_norms_exact(off):
    """Integer patterns (the first exact step: w and g = w in {0, +-1, +-2}): every partial sum is an integer up to
    2^24, so the sums are equal in any order of summation. Views at element offsets 0..3 past a 16-byte boundary; at
    offset 0 also the layer whose partials need the finish wave's second trip. (From the second step on w is a
    dyadic multiple c w0: the layer sums c^2 4^a are still fp32 numbers, the partial sums on the way are not.)"""
    lengths = lc.LENGTHS + ((lc.FINISH_SECOND_TRIP,) if off == 0 else ())
    pieces, n, w0, hp, rate_num, steps, exact = lc.exact_run(lengths, 1.0, (1.0, -3.0), seed=20 + off, base=off)
    assert exact
    ar = _Arena()
    b = _Bufs(ar, pieces, len(pieces), n, off)
    w = ar.put(w0.to(F32), off)
    g64, acc64 = steps[0][0], steps[0][1]
    assert lc.is_f32(acc64) and bool((acc64 == acc64.round()).all())
    got = b.norms(w, ar.put(g64.to(F32), off))
    assert torch.equal(got.cpu().to(F64), acc64)
    # an unrelated integer gradient pattern of the same norm against the same w
    g2 = torch.zeros(n, dtype=F64)
    for k, (lo, hi, _) in enumerate(pieces):
        g2[lo:hi] = lc.square_vec(hi - lo, 900 + k)[0]
    got = b.norms(w, ar.put(g2.to(F32), off))
    assert torch.equal(got.cpu().to(F64), lc.sums_oracle(w0, g2, pieces, len(pieces)))
    assert ar.ok()


def test_norms_gaussian_within_the_chain_bound_and_reproducible():
    pieces, n, w, g, v, hp, rate_num = lc.gauss_case(lc.LENGTHS + (lc.FINISH_SECOND_TRIP,), seed=31, base=1)
    ar = _Arena()
    b = _Bufs(ar, pieces, len(pieces), n, 0)
    wd, gd = ar.put(w), ar.put(g)
    first = b.norms(wd, gd).clone()
    b.ws.fill_(float("nan"))                       # neither kernel may depend on what the workspace or acc held
    second = ar.new(2 * len(pieces), F32)
    second.fill_(float("nan"))
    b.norms(wd, gd, second)
    assert st.same_bits(first, second)
    want = lc.sums_oracle(w, g, pieces, len(pieces))
    got = first.cpu().to(F64)
    for lo, hi, layer in pieces:
        for j, what in ((0, "w"), (1, "g")):
            t = float(want[2 * layer + j])
            r = abs(float(got[2 * layer + j]) - t) / lc.norm_bound(t, lc.chunks_of(pieces, layer))
            assert _report("norm", f"n={hi - lo} {what}", r) <= ALLOWED["norm"], (hi - lo, what, r)
    assert ar.ok()


def test_norms_of_a_layer_without_a_chunk_are_zero():
    pieces = [(0, 5, 0), (5, 5 + C + 1, 2)]                   # layer 1 belongs to another rank
    ar = _Arena()
    b = _Bufs(ar, pieces, 3, 5 + C + 1)
    b.acc.fill_(float("nan"))
    x = ar.put(torch.ones(5 + C + 1, dtype=F32))
    got = b.norms(x, x).cpu()
    assert got.tolist() == [5.0, 5.0, 0.0, 0.0, C + 1.0, C + 1.0]
    assert ar.ok()


# ================================================================================================== update
def _update_exact(lengths, WD, betas, off, seed, first_step=0):
    pieces, n, w0, hp, rate_num, steps, exact = lc.exact_run(lengths, WD, betas, seed, base=off)
    assert exact
    ar = _Arena()
    b = _Bufs(ar, pieces, len(pieces), n, off)
    w = ar.put((w0 if first_step == 0 else steps[first_step - 1][2]).to(F32), off)
    w16 = ar.new(n, BF, off)
    w16.copy_(w)
    shadow0 = w16.clone()
    b.put_v((torch.zeros(n, dtype=F64) if first_step == 0 else steps[first_step - 1][3]).to(F32).to(DEV))
    for s, (g64, acc64, we, ve) in enumerate(steps):
        if s < first_step:
            continue
        g = ar.put(g64.to(F32), off)
        b.update(w, g, w16, hp, rate_num, _acc32(acc64), WD)
        assert torch.equal(w.cpu().to(F64), we), s
        assert torch.equal(b.get_v(torch.zeros(n, dtype=F32)).to(F64), ve), s
        want16 = shadow0.clone().cpu()
        for lo, hi, _ in pieces:
            want16[lo:hi] = we[lo:hi].to(F32).to(BF)
        assert st.same_bits(w16.cpu(), want16), s            # rounded inside the pieces, untouched outside
    assert ar.ok()


@pytest.mark.parametrize("off", (0, 1, 2, 3))
@pytest.mark.parametrize("WD,betas", lc.EXACT_WD)
def test_update_exact_three_steps(WD, betas, off):
    """acc is given (the oracle's sums): scale is 1, 2 or 4 and every intermediate an fp32 number, so w, v and the
    bf16 shadow equal the fp64 oracle after each of three steps."""
    lengths = lc.LENGTHS + ((lc.FINISH_SECOND_TRIP,) if off == 0 else ())
    _update_exact(lengths, WD, betas, off, seed=40 + off)


def test_norms_and_update_past_the_block_cap():
    """More chunks than blocks: the grid-stride loops of both kernels take a second trip. The last exact step (w and
    g unrelated patterns) from the oracle's state before it."""
    pieces, n, w0, hp, rate_num, steps, exact = lc.exact_run(lc.PAST_CAP_LENGTHS, 1.0, (1.0, -3.0), seed=50)
    assert exact and sum(lc.chunks_of(pieces, ly) for ly in range(len(pieces))) > lc.BLOCK_CAP
    ar = _Arena()
    b = _Bufs(ar, pieces, len(pieces), n)
    w, g = ar.put(w0.to(F32)), ar.put(steps[0][0].to(F32))
    assert torch.equal(b.norms(w, g).cpu().to(F64), steps[0][1])        # integer partial sums: exact
    g64, acc64, we, ve = steps[2]
    w.copy_(steps[1][2].to(F32))
    g.copy_(g64.to(F32))
    w16 = ar.new(n, BF)
    b.put_v(steps[1][3].to(F32).to(DEV))
    b.update(w, g, w16, hp, rate_num, _acc32(acc64), 1.0)
    assert torch.equal(w.to(F64), we.to(DEV))
    assert torch.equal(b.get_v(torch.zeros(n, dtype=F32)).to(F64), ve)
    assert torch.equal(w16, w.to(BF))
    assert ar.ok()


def _gauss_check(tag, w, v_got, w16, pieces, we, ve, mag, widen=None):
    """ulp distances of w and v over the pieces; the shadow is the correctly rounded bf16 of the kernel's own w."""
    for k, (lo, hi, _) in enumerate(pieces):
        extra = 0.0 if widen is None else widen[k]
        for name, got, want, m in (("update_w", w[lo:hi], we[lo:hi], mag["w"][lo:hi]),
                                   ("update_v", v_got[lo:hi], ve[lo:hi], mag["v"][lo:hi])):
            if extra:
                err = (got.to(F64) - want).abs()
                lim = ALLOWED[name] * st.ulp32(torch.maximum(want.abs(), m)) + extra * mag["step"][lo:hi]
                assert bool((err <= lim).all()), (tag, name, k, float((err / lim).max()))
            else:
                d = _report(name, f"{tag} n={hi - lo}", st.ulp_dist(got, want, mag=m))
                assert d <= ALLOWED[name], (tag, name, k, d)
        assert st.same_bits(w16[lo:hi], w[lo:hi].to(BF)), (tag, k)


@pytest.mark.parametrize("off", (0, 1, 2, 3))
def test_update_gaussian(off):
    lengths = lc.LENGTHS + ((lc.FINISH_SECOND_TRIP,) if off == 0 else ())
    pieces, n, w, g, v, hp, rate_num = lc.gauss_case(lengths, seed=60 + off, base=off)
    acc = lc.sums_oracle(w, g, pieces, len(pieces)).to(F32)
    ar = _Arena()
    b = _Bufs(ar, pieces, len(pieces), n, off)
    wd, gd, w16 = ar.put(w, off), ar.put(g, off), ar.new(n, BF, off)
    b.put_v(v.to(DEV))
    b.update(wd, gd, w16, hp, rate_num, acc.to(DEV), lc.GAUSS_WD)
    we, ve, mag = lc.update_oracle(w, g, v, pieces, _hp32(hp), _f32s(rate_num), acc, lc.GAUSS_WD)
    _gauss_check(f"off={off}", wd.cpu(), b.get_v(v), w16.cpu(), pieces, we, ve, mag)
    assert torch.equal(wd.cpu()[:off], w[:off])               # elements before the first piece are not touched
    assert ar.ok()


@pytest.mark.parametrize("name", sorted(lc.guard_cases()))
def test_guards_through_the_update(name):
    """inf -> 1e4, nan -> 1, ~0 -> 1e-4 and a NaN gradient, from the norm kernels' own sums through the update."""
    w, g, WD, want_scale = lc.guard_cases()[name]
    n = w.numel()
    pieces, hp, rate_num = [(0, n, 0)], [(1e-4, 0.9)], [0.05]
    v = (1e-3 * torch.randn(n, generator=st.gen(12))).to(F32)
    ar = _Arena()
    b = _Bufs(ar, pieces, 1, n)
    wd, gd, w16 = ar.put(w), ar.put(g), ar.new(n, BF)
    b.put_v(v.to(DEV))
    acc = b.norms(wd, gd)
    b.update(wd, gd, w16, hp, rate_num, acc, WD)
    acc_host = acc.cpu()
    assert float(lc.scale_oracle(acc_host, WD)[0]) == want_scale
    we, ve, mag = lc.update_oracle(w, g, v, pieces, _hp32(hp), _f32s(rate_num), acc_host, WD)
    got_w, got_v = wd.cpu(), b.get_v(v)
    nan = torch.isnan(we)
    assert torch.equal(torch.isnan(got_w), nan) and torch.equal(torch.isnan(got_v), torch.isnan(ve))
    assert int(nan.sum()) == (1 if name == "nan_g" else 0)
    keep = ~nan
    for nm, got, want, m in (("update_w", got_w, we, mag["w"]), ("update_v", got_v, ve, mag["v"])):
        d = _report(nm, f"guard {name}", st.ulp_dist(got[keep], want[keep], mag=m[keep]))
        assert d <= ALLOWED[nm], (name, nm, d)
    assert torch.equal(torch.isnan(w16.cpu().float()), nan) and st.same_bits(w16.cpu()[keep], got_w[keep].to(BF))
    if name == "zero_w_zero_g":                       # the update is zero: w stays 0, v only decays
        assert torch.equal(got_w, -got_v) and torch.equal(got_v, torch.tensor(0.9, dtype=F32) * v)
    assert ar.ok()


# ================================================================================================== two ranks
def _cuts(pieces):
    return (pieces[4][0] + 5, pieces[6][1], pieces[-1][0] + C + 17)


def test_two_rank_split_exact():
    """Rank A's and rank B's pieces (cut inside layers, off the chunk grid; some layers wholly on one side): on
    integer data the two acc vectors add up to the one-plan sums, and the two updates give the one-plan result bit
    for bit over three steps."""
    pieces, n, w0, hp, rate_num, steps, exact = lc.exact_run(lc.LENGTHS, 1.0, (1.0, -3.0), seed=70)
    assert exact
    L = len(pieces)
    sides = lc.split_two(pieces, _cuts(pieces))
    ar = _Arena()
    one = _Bufs(ar, pieces, L, n)
    ranks = [_Bufs(ar, s, L, n) for s in sides]
    w1, w2 = ar.put(w0.to(F32)), ar.put(w0.to(F32))
    s1, s2 = ar.new(n, BF), ar.new(n, BF)
    one.put_v(torch.zeros(n, device=DEV))
    for r in ranks:
        r.put_v(torch.zeros(n, device=DEV))
    for s, (g64, acc64, we, ve) in enumerate(steps):
        g = ar.put(g64.to(F32))
        total = ranks[0].norms(w2, g).clone() + ranks[1].norms(w2, g)        # as the all-reduce adds them
        if s == 0:                          # integer partial sums: the split sums add up to the one-plan sums
            assert torch.equal(total.cpu().to(F64), acc64) and st.same_bits(total, one.norms(w1, g))
        total = _acc32(acc64)               # the updates take the given sums, as the exact legs do
        one.update(w1, g, s1, hp, rate_num, total, 1.0)
        for r, side in zip(ranks, sides):
            r.update(w2, g, s2, [hp[ly] for _, _, ly in side], [rate_num[ly] for _, _, ly in side], total, 1.0)
        assert st.same_bits(w1, w2) and st.same_bits(s1, s2) and torch.equal(w1.cpu().to(F64), we)
        v2 = torch.zeros(n, dtype=F32)
        for r in ranks:
            v2 = r.get_v(v2)
        assert st.same_bits(one.get_v(torch.zeros(n, dtype=F32)), v2)
    assert ar.ok()


def test_two_rank_split_gaussian():
    pieces, n, w, g, v, hp, rate_num = lc.gauss_case(lc.LENGTHS, seed=71)
    L = len(pieces)
    sides = lc.split_two(pieces, _cuts(pieces))
    ar = _Arena()
    ranks = [_Bufs(ar, s, L, n) for s in sides]
    wd, gd, w16 = ar.put(w), ar.put(g), ar.new(n, BF)
    total = ranks[0].norms(wd, gd).clone() + ranks[1].norms(wd, gd)
    for r, side in zip(ranks, sides):
        r.put_v(v.to(DEV))
        r.update(wd, gd, w16, [hp[ly] for _, _, ly in side], [rate_num[ly] for _, _, ly in side], total, lc.GAUSS_WD)
    we, ve, mag = lc.update_oracle(w, g, v, pieces, _hp32(hp), _f32s(rate_num), total.cpu(), lc.GAUSS_WD)
    v_got = v.clone()
    for r in ranks:
        v_got = r.get_v(v_got)
    _gauss_check("two ranks", wd.cpu(), v_got, w16.cpu(), pieces, we, ve, mag)
    want = lc.sums_oracle(w, g, pieces, L)
    for ly in range(L):                       # two partial sums and their fp32 addition: one more rounding
        for j in (0, 1):
            t = float(want[2 * ly + j])
            bound = lc.norm_bound(t, lc.chunks_of(pieces, ly)) + st.U24 * t
            assert abs(float(total[2 * ly + j]) - t) <= ALLOWED["norm"] * bound
    assert ar.ok()


# ================================================================================================== TrainStep
SIZES = ((40, 70), (70, 1100), (1100, 3))            # the middle layer spans 19 chunks
LR, TRUST, WDECAY, MOM = 0.1, 0.02, 1e-3, 0.9


def _model():
    from bigdl_amd import nn
    from bigdl_amd.utils.random_generator import RNG

    RNG.setSeed(9)
    m = nn.Sequential().setName("net")
    for i, (a, b) in enumerate(SIZES):
        m.add(nn.Linear(a, b).setName(f"fc{i + 1}"))
    return m


def _poly():
    from bigdl_amd.optim.sgd import Poly

    return Poly(0.5, 100)


def _poly_rate(s):
    return LR * (1.0 - s / 100) ** 0.5


def _train_step(methods, expand=False):
    from bigdl_amd import nn
    from bigdl_amd.optim.train_step import TrainStep

    return TrainStep(_model(), nn.MSECriterion(), methods, device=DEV, expand_methods=expand)


def _norm_widen(n):
    """Relative error the kernels' own sums may put on the rate: each norm half of its sum's, two norms."""
    eps = ALLOWED["norm"] * lc.norm_chain((n + C - 1) // C) * st.U24
    return eps


def _tail(step, loss=0.0):
    with no_sync():
        step.apply_processors()
        step.optimize_pieces(loss)


def _run_steps(step, lars_names, sgd=None, first=0, steps=3):
    """Inject gradients, run the tail, and hold every step to the oracle taken from the device state before it."""
    pieces = [(p.lo, p.hi, lars_names.index(p.name)) for p in step.plan if p.name in lars_names]
    meths = [p.method for p in step.plan if p.name in lars_names]
    n = step.w.numel()
    hp = [(WDECAY, MOM)] * len(pieces)
    for s in range(first, first + steps):
        given = (0.01 * torch.randn(n, generator=st.gen(80 + s))).to(F32)
        step.g.copy_(given)
        w_before = step.w.cpu().clone()
        v_before = torch.zeros(n, dtype=F32)
        for (lo, hi, _), m in zip(pieces, meths):
            sv = m.state.get("v")
            if sv is not None:
                v_before[lo:hi] = sv.cpu()
        _tail(step)
        rate_num = [_poly_rate(s) * TRUST] * len(pieces)
        acc = lc.sums_oracle(w_before, given, pieces, len(lars_names))
        we, ve, mag = lc.update_oracle(w_before, given, v_before, pieces, _hp32(hp), _f32s(rate_num), acc, WDECAY)
        w_got, w16 = step.w.cpu(), step.w16.cpu()
        v_got = torch.zeros(n, dtype=F32)
        for (lo, hi, _), m in zip(pieces, meths):
            assert m.state["v"].numel() == hi - lo
            v_got[lo:hi] = m.state["v"].cpu()
        _gauss_check(f"step {s}", w_got, v_got, w16, pieces, we, ve, mag, widen=[_norm_widen(hi - lo) for lo, hi, _ in pieces])
        if sgd is not None:
            for p in step.plan:
                if p.name in lars_names:
                    continue
                lr = sgd
                want, _ = st.sgd_oracle(w_before[p.lo:p.hi], given[p.lo:p.hi], None, lr, 0.0, 0.0, 0.0, False, True)
                m = st.sgd_mags(w_before[p.lo:p.hi], given[p.lo:p.hi], None, lr, 0.0, 0.0, 0.0, False, True)["w"]
                assert st.ulp_dist(w_got[p.lo:p.hi], want, mag=m) <= SGD_W_ALLOWED, p.name
                assert st.same_bits(w16[p.lo:p.hi], w_got[p.lo:p.hi].to(BF)), p.name
    return pieces, meths


def _kernel_launches(fn):
    """Names of the device kernels ``fn`` launches (copies and memsets are not kernels)."""
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
            and not e.name.lower().startswith(("memcpy", "memset", "copy"))]


def _lars_methods(model):
    from bigdl_amd.optim.methods import LarsSGD

    return LarsSGD.createOptimForModule(model, _poly(), TRUST, LR, 0.0, WDECAY, MOM)


def test_train_step_fused_route():
    from bigdl_amd.optim.methods import LarsSGD
    from bigdl_amd.optim.train_step import TrainStep
    from bigdl_amd import nn

    names = [f"fc{i + 1}" for i in range(len(SIZES))]
    with switch(True):
        model = _model()
        step = TrainStep(model, nn.MSECriterion(), _lars_methods(model), device=DEV)
        assert step.lars_plan is not None
        pieces, meths = _run_steps(step, names)
        assert lars.last_route() == "fused"
        assert all(isinstance(m, LarsSGD) and m._calculated_scale is None for m in meths)
        # every method's state is a view of the plan's momentum buffer (getState / checkpoints read it there)
        base, end = step.lars_plan.vbuf.data_ptr(), step.lars_plan.vbuf.data_ptr() + 4 * step.lars_plan.vbuf.numel()
        assert all(base <= m.state["v"].data_ptr() < end for m in meths)
        step.g.copy_((0.01 * torch.randn(step.g.numel(), generator=st.gen(90))).to(F32))
        kernels = _kernel_launches(lambda: (step.apply_processors(), step.optimize_pieces(0.0)))
        assert len(kernels) == 3 and all("lars_" in k for k in kernels), kernels


def test_train_step_switch_off_takes_the_loop():
    from bigdl_amd import nn
    from bigdl_amd.optim.train_step import TrainStep

    with switch(False):
        model = _model()
        step = TrainStep(model, nn.MSECriterion(), _lars_methods(model), device=DEV)
        assert step.lars_plan is None
        step.g.copy_((0.01 * torch.randn(step.g.numel(), generator=st.gen(91))).to(F32))
        step.apply_processors()
        step.optimize_pieces(0.0)
        assert lars.last_route() == "loop"
        assert bool(torch.isfinite(step.w).all())


def test_train_step_state_set_by_hand_is_honoured():
    from bigdl_amd import nn
    from bigdl_amd.optim.train_step import TrainStep

    names = [f"fc{i + 1}" for i in range(len(SIZES))]
    with switch(True):
        model = _model()
        step = TrainStep(model, nn.MSECriterion(), _lars_methods(model), device=DEV)
        _run_steps(step, names, steps=1)
        p = step.plan[1]
        mine = (1e-3 * torch.randn(p.hi - p.lo, generator=st.gen(92))).to(F32).to(DEV)
        p.method.state["v"] = mine                       # as a loaded checkpoint would
        step.plan[2].method.clearHistory()               # and a cleared one starts from zero
        _run_steps(step, names, first=1, steps=1)        # reads state["v"] before the step: the oracle starts there
        assert p.method.state["v"].data_ptr() != mine.data_ptr()
        assert lars.last_route() == "fused"


def test_train_step_mixed_plan():
    from bigdl_amd import nn
    from bigdl_amd import optim as O
    from bigdl_amd.optim.methods import LarsSGD
    from bigdl_amd.optim.train_step import TrainStep

    with switch(True):
        model = _model()
        methods = {"fc1": O.SGD(0.05), "fc2": LarsSGD(_poly(), TRUST, LR, 0.0, WDECAY, MOM), "fc3": O.SGD(0.05)}
        step = TrainStep(model, nn.MSECriterion(), methods, device=DEV)
        assert step.lars_plan is not None and len(step.lars_plan.methods) == 1
        _run_steps(step, ["fc2"], sgd=0.05)
        assert lars.last_route() == "fused"


def test_train_step_expanded_from_one_inherited_method():
    from bigdl_amd import nn
    from bigdl_amd.optim.methods import LarsSGD
    from bigdl_amd.optim.train_step import TrainStep

    names = [f"fc{i + 1}" for i in range(len(SIZES))]
    with switch(True):
        model = _model()
        step = TrainStep(model, nn.MSECriterion(), {"net": LarsSGD(_poly(), TRUST, LR, 0.0, WDECAY, MOM)}, device=DEV,
                         expand_methods=True)
        assert [s[0] for s in step.splits] == names and step.lars_plan.nlayers == 3
        _run_steps(step, names)                           # the per-layer result: every leaf is its own layer
        assert lars.last_route() == "fused"


# ================================================================================================== stand-alone
@pytest.mark.parametrize("off", (0, 3))
def test_stand_alone_optimize(off):
    from bigdl_amd.optim.methods import LarsSGD

    n = 2 * C + 3
    q = st.gen(95)
    w = (0.1 * torch.randn(n, generator=q)).to(F32)
    ar = _Arena()
    x, w16 = ar.put(w, off), ar.new(n, BF, off)
    with switch(True):
        m = LarsSGD(_poly(), TRUST, LR, 0.0, WDECAY, MOM).attach_shadow(w16)
        v = torch.zeros(n, dtype=F32)
        for s in range(2):
            g = (0.01 * torch.randn(n, generator=q)).to(F32)
            gd = ar.put(g, off)
            w_before = x.cpu().clone()
            with no_sync():
                m.optimize(lambda _x: (0.0, gd), x)
            assert lars.last_route() == "fused"
            pieces = [(0, n, 0)]
            acc = lc.sums_oracle(w_before, g, pieces, 1)
            we, ve, mag = lc.update_oracle(w_before, g, v, pieces, _hp32([(WDECAY, MOM)]),
                                           _f32s([_poly_rate(s) * TRUST]), acc, WDECAY)
            v = m.state["v"].cpu()
            _gauss_check(f"stand-alone {s}", x.cpu(), v, w16.cpu(), pieces, we, ve, mag, widen=[_norm_widen(n)])
    assert ar.ok()


def test_bindings_reject_buffers_of_different_phase():
    ar = _Arena()
    b = _Bufs(ar, [(0, 8, 0)], 1, 8)
    w, g = ar.new(8, F32, 0), ar.new(8, F32, 1)
    with pytest.raises(RuntimeError, match="phase"):
        b.norms(w, g)
    with pytest.raises(RuntimeError, match="shorter"):
        b.norms(ar.new(4, F32), ar.new(4, F32))
