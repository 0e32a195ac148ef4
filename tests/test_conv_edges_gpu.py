"""The convolution kernels against tests/conv_edge_cases.py, element by element, on every dispatch route.

Each case first asserts, through conv_nt_plan_info / conv_wgrad_plan_info (nothing is launched), that the route its
row names is the one the call takes under the row's switches; then runs two legs:

* exact: integer data, ``torch.equal`` on the whole output against the fp64 result rounded to nearest even, and the
  fused reductions against fp64 sums over the *expected* output (equality where provable, else the summation bound);
* gauss: bf16 Gaussian data, every element within 2^-8 |ref| + 2 Kdim 2^-24 A.

BIGDL_CONV_EDGE_PROFILE=<file> writes the largest observed ratio to each bound, per route (profiles/
conv_edge_errors.txt is such a file)."""
import contextlib
import os

import pytest
import torch

from tests import conv_edge_cases as ce

pytestmark = pytest.mark.gpu

CL = torch.channels_last
BF = torch.bfloat16
RATIOS = {}          # (route, kind) -> largest observed ratio to the bound


def _C():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bigdl_amd.ops import native

    return native.get()


@pytest.fixture(scope="module", autouse=True)
def _profile():
    yield
    path = os.environ.get("BIGDL_CONV_EDGE_PROFILE")
    if path and RATIOS:
        with open(path, "w") as f:
            f.write("# tests/test_conv_edges_gpu.py with BIGDL_CONV_EDGE_PROFILE set, on one MI355X.\n"
                    "# route, check, largest observed |got - ref| / bound over the route's cases (<= 1 passes):\n"
                    "# gauss = Gaussian-leg outputs (2^-8 |ref| + 2 Kdim 2^-24 A; RNE alone reaches just under 1),\n"
                    "# sum1 / sum2 = the fused reductions of the exact leg where equality is not provable,\n"
                    "# gauss_dw / gauss_db = weight and bias gradients (2^-23 |ref| + 2 M 2^-24 A)\n")
            for (route, kind), r in sorted(RATIOS.items()):
                f.write(f"{route:16s} {kind:10s} {r:.4f}\n")


def _note(route, kind, ratio):
    RATIOS[(route, kind)] = max(RATIOS.get((route, kind), 0.0), float(ratio))


@contextlib.contextmanager
def switches(C_, case):
    """Run under the table's baseline plus the row's own settings; put back what was found on entry."""
    found = {name: getattr(C_, "get_" + name[4:])() for name in ce.DEFAULT_SWITCHES}
    try:
        for name, v in {**ce.DEFAULT_SWITCHES, **dict(case.sw)}.items():
            getattr(C_, name)(v)
        yield
    finally:
        torch.cuda.synchronize()
        for name, v in found.items():
            getattr(C_, name)(v)


def _bf(t, cl=True):
    t = t.to(BF).cuda()
    return t.contiguous(memory_format=CL) if cl else t.contiguous()


def _f32(t):
    return t.float().cuda().contiguous()


def _sign_mask(z):
    """[P][C / 8] uint8 sign bytes of an NCHW tensor in NHWC order (bit e of byte (p, g): z[p][8 g + e] > 0)."""
    N, C, H, W = z.shape
    b = (z.permute(0, 2, 3, 1).reshape(-1, C // 8, 8) > 0).to(torch.int32)
    return (b * (1 << torch.arange(8, dtype=torch.int32))).sum(-1).to(torch.uint8).reshape(-1).contiguous().cuda()


def _kernel(plan):
    """Profile key of a conv_nt_plan_info answer: the kernel, with its tile and stage form where it has several."""
    return plan[0] if plan[0] != "g4" else "g4_%dx%dx%d" % tuple(plan[1:4])


# ------------------------------------------------------------------------------------------------------------------
# forward / data gradient
# ------------------------------------------------------------------------------------------------------------------
def _fwd_geo(case):
    from bigdl_amd.ops import conv as cv

    N, C, H, K, R, st, pd, OH = case.dims
    if case.pair:
        geo = [N, ce.STEM_HP, ce.STEM_WQ, 8, ce.STEM_OH, ce.STEM_OW, 2, 1, 224, K, K, ce.STEM_OH, ce.STEM_OW, 1, 1, 0, 0]
        return geo, cv._pair_taps(7, ce.STEM_S2)
    return cv._fwd_geo(N, H, case.W, C, OH, case.OW, st, st, R * R * C, K), cv._fwd_taps(R, R, pd, pd, 1, 1)


def _phases(case):
    from bigdl_amd.ops import conv as cv

    N, C, H, K, R, st, pd, OH = case.dims
    return cv.dgrad_phases(H, case.W, R, R, (st, st), (pd, pd), (1, 1))


def nt_plans(C_, case):
    """[(what, plan reported, plan wanted)] for every GEMM the case launches."""
    out = []
    geo, taps = _fwd_geo(case)
    for op in ce.fwd_ops(case):
        g = list(geo)
        if op == "slice_bias_stats":
            g[10] = g[9] + 2 * case.slice                 # ldo: the row stride of the wider buffer
        out.append((op, tuple(C_.conv_nt_plan_info(g, taps, ce.op_flags(op)))[:4], case.fwd))
    if case.dgrad and case.dgrad != "s2":
        N, C, H, K, R, st, pd, OH = case.dims
        assert ce.covered(case) == (sum(nI * nJ for (_, _, nI, nJ, _) in _phases(case)) == H * case.W)
        for op in ce.dgrad_ops(case):
            for (a, b, nI, nJ, ptaps) in _phases(case):
                g = [N, OH, case.OW, K, nI, nJ, 1, 1, R * R * K, C, C, H, case.W, st, st, a, b]
                got = C_.conv_nt_plan_info(g, ptaps, ce.op_flags(op), [2, 2] if op.startswith("sub_") else [])
                out.append((f"{op} phase {a}{b}", tuple(got)[:4], case.dgrad))
    return out


def _compare(case, leg, op, got, route, fp32_out=False):
    """``got``: NCHW tensor on the GPU. Exact leg: equal to the rounded reference, bit for bit; returns the expected
    tensor. Gaussian leg: every element within its bound."""
    ref, A = ce.nt_exact(case, leg, op)
    got = got.cpu()
    assert got.shape == ref.shape
    if leg == "int":
        want = ref.float() if fp32_out else ce.round_bf16(ref)
        if not torch.equal(got, want):
            bad = (got.double() != want.double())
            rows = bad.any(dim=1).nonzero()
            pytest.fail(f"{case} {op}: {int(bad.sum())} of {bad.numel()} elements differ, in {len(rows)} pixels; "
                        f"first {bad.nonzero()[0].tolist()}: got {got[bad][0].item()} want {want[bad][0].item()}")
        return want
    bound = (2.0 ** -23 * ref.abs() + 2 * case.kdim_fwd * ce.U24 * A) if fp32_out else ce.nt_bound(case, op, ref, A)
    ratio = ((got.double() - ref).abs() / bound.clamp_min(1e-300)).max().item()
    _note(route, "gauss", ratio)
    assert ratio <= 1.0, f"{case} {op}: |got - ref| reaches {ratio:.3f} of the per-element bound"
    return None


def _check_reduction(C_, case, leg, op, buf, want16, route):
    if leg != "int":
        return
    ch = want16.shape[1]
    got = buf.view(C_.STAT_SLOTS, 2, ch).double().sum(0).cpu()
    for i, (s, exact, bound) in enumerate(ce.reduction_ref(case, leg, op, want16)):
        diff = (got[i] - s).abs()
        assert torch.equal(got[i][exact], s[exact]), \
            f"{case} {op}: sum {i + 1} differs on {int((diff[exact] != 0).sum())} exactly summable channels"
        if (~exact).any():
            ratio = (diff[~exact] / bound[~exact].clamp_min(1e-300)).max().item()
            _note(route, f"sum{i + 1}", ratio)
            assert ratio <= 1.0, f"{case} {op}: sum {i + 1} off by {ratio:.3f} of the summation bound"


def _run_fwd(C_, case, leg, op):
    from bigdl_amd.ops import conv as cv

    N, C, H, K, R, st, pd, OH = case.dims
    d = ce.nt_inputs(case, leg)
    bias = _f32(d["bias"])
    stats = torch.zeros(C_.STAT_SLOTS * 2 * K, device="cuda") if op.endswith("stats") else None
    relu = op == "bias_relu"
    if case.pair:
        xp, wp = _bf(ce.to_pairs(d["x"]), cl=False), _bf(ce.pair_weight(d["w"]), cl=False)
        y = cv.conv2d_pairs_fwd(xp, wp, bias, K, ce.STEM_OH, ce.STEM_OW, 7, ce.STEM_S2, 2, relu=relu, stats=stats)
    elif op == "out32_acc":
        geo, taps = _fwd_geo(case)
        out = _f32(d["out0"].permute(0, 2, 3, 1))                 # [N][OH][OW][K] fp32, accumulated into
        C_.conv_nt(_bf(d["x"]), _bf(d["w"]), out, None, None, geo, taps, False, accumulate=True)
        _compare(case, leg, op, out.permute(0, 3, 1, 2), _kernel(case.fwd), fp32_out=True)
        return
    elif op == "slice_bias_stats":
        c0 = case.slice
        buf = torch.full((N, K + 2 * c0, OH, case.OW), 7.0, dtype=BF, device="cuda").contiguous(memory_format=CL)
        y = cv.conv2d_fwd(_bf(d["x"]), _bf(d["w"]), bias, (st, st), (pd, pd), stats=stats, out=buf[:, c0:c0 + K])
        torch.cuda.synchronize()
        assert (buf[:, :c0] == 7).all() and (buf[:, c0 + K:] == 7).all(), f"{case}: wrote outside its channel slice"
    elif op == "pre_bias_stats":
        y, mat = cv.conv2d_fwd(_bf(d["x"]), _bf(d["w"]), bias, (st, st), (pd, pd), stats=stats, pre=_f32(d["pre"]))
        assert mat is None, "the BN was materialised instead of applied on load"
    else:
        y = cv.conv2d_fwd(_bf(d["x"]), _bf(d["w"]), bias, (st, st), (pd, pd), relu=relu, stats=stats)
    torch.cuda.synchronize()
    want16 = _compare(case, leg, op, y, _kernel(case.fwd))
    if stats is not None:
        _check_reduction(C_, case, leg, op, stats, want16, _kernel(case.fwd))


def _run_dgrad(C_, case, leg, op):
    from bigdl_amd.ops import conv as cv

    N, C, H, K, R, st, pd, OH = case.dims
    d = ce.nt_inputs(case, leg)
    dy = _bf(d["dy"])
    wt = _bf(d["w"].permute(1, 2, 3, 0), cl=False)                # (C, R, S, K)
    route = "halo_s2" if case.dgrad == "s2" else _kernel(case.dgrad)
    bn = red = None
    if op != "add":
        mask = op.rsplit("_", 1)[1]
        red = torch.zeros(C_.STAT_SLOTS * 2 * C, device="cuda")
        bn = {"x": _bf(d["bx"]), "z": _bf(d["bz"]) if mask == "z" else None,
              "zm": _sign_mask(d["bz"]) if mask == "zm" else None, "mean": _f32(d["mean"]), "aff": _f32(d["aff"]),
              "red": red}
    addend = None
    if op.startswith("add"):
        addend = _bf(d["addend"])
    elif op.startswith("sub_"):
        assert cv.addend_stride_applies(N, K, H, case.W, C, (2, 2), bn=1)
        addend = _bf(d["sub"])
        addend._compact_stride = (2, 2)
    if case.dgrad == "s2":
        dx = torch.empty((N, C, H, case.W), dtype=BF, device="cuda").contiguous(memory_format=CL)
        bnk = dict(bn_x=bn["x"], bn_z=bn["z"], bn_mean=bn["mean"], bn_aff=bn["aff"], bn_red=bn["red"], bn_zm=bn["zm"])
        assert C_.dgrad_s2_applies(dy, wt, dx, **bnk), "the one-pass stride-2 data gradient declines the case"
        assert C_.dgrad_s2(dy, wt, dx, **bnk)
    else:
        dx = cv.conv2d_dgrad(dy, wt, (N, C, H, case.W), (st, st), (pd, pd), addend=addend, bn=bn)
        assert bn is None or bn.get("done"), "the consumer-BN reduction was not fused"
    torch.cuda.synchronize()
    want16 = _compare(case, leg, op, dx, route)
    if red is not None:
        _check_reduction(C_, case, leg, op, red, want16, route)


@pytest.mark.parametrize("case", ce.NT_CASES, ids=str)
def test_conv_nt_route_matches_reference(case):
    C_ = _C()
    with switches(C_, case):
        for what, got, want in nt_plans(C_, case):
            assert got == want, f"{case} {what}: runs {got}, the row names {want}"
        for leg in ("int", "gauss"):
            for op in ce.fwd_ops(case):
                _run_fwd(C_, case, leg, op)
            for op in ce.dgrad_ops(case):
                _run_dgrad(C_, case, leg, op)


# ------------------------------------------------------------------------------------------------------------------
# weight gradient
# ------------------------------------------------------------------------------------------------------------------
def _wg_geo(case):
    N, C, H, K, R, st, pd, OH = case.dims
    if case.pair:
        return [N, ce.STEM_HP, ce.STEM_WQ, 8, ce.STEM_OH, ce.STEM_OW, 7, ce.STEM_S2, 2, 1, 0, 0, 1, 1,
                N * ce.STEM_OH * ce.STEM_OW, K, 224, K]
    return [N, H, case.W, C, OH, case.OW, R, R, st, st, pd, pd, 1, 1, N * OH * case.OW, K, R * R * C, K]


def wg_plan(C_, case, bias):
    """(kernel, splits) conv_wgrad takes: the chooser's own answers (conv_wgrad_plan_name, conv_wgrad_plan_info)."""
    return C_.conv_wgrad_plan_name(_wg_geo(case), bias), C_.conv_wgrad_plan_info(_wg_geo(case), bias)[0]


def _wg_compare(case, leg, what, got, ref, A, kind):
    got = got.cpu()
    if leg == "int":
        want = ref.float()
        if not torch.equal(got, want):
            bad = got != want
            pytest.fail(f"{case} {what}: {int(bad.sum())} of {bad.numel()} elements differ; first "
                        f"{bad.nonzero()[0].tolist()}: got {got[bad][0].item()} want {want[bad][0].item()}")
        return
    ratio = ((got.double() - ref).abs() / ce.wg_bound(case, ref, A).clamp_min(1e-300)).max().item()
    _note("wgrad_" + case.kernel, kind, ratio)
    assert ratio <= 1.0, f"{case} {what}: |got - ref| reaches {ratio:.3f} of the per-element bound"


@pytest.mark.parametrize("case", ce.WG_CASES, ids=str)
def test_conv_wgrad_route_matches_reference(case):
    from bigdl_amd.ops import conv as cv

    C_ = _C()
    N, C, H, K, R, st, pd, OH = case.dims
    with switches(C_, case):
        for bias in (True, False):
            assert wg_plan(C_, case, bias) == (case.kernel, case.splits), (bias, wg_plan(C_, case, bias))
        for leg in ("int", "gauss"):
            d = ce.wg_inputs(case, leg)
            dwr, dbr, Aw, Ab = ce.wg_reference(case, leg)
            for bias in (True, False):
                for tr_asm in (1, 0):          # same kernels behind a template flag: both must meet the reference
                    C_.set_wgrad_tr_asm(tr_asm)
                    db = _f32(d["db0"]) if bias else None
                    what = f"{leg} bias={bias} tr_asm={tr_asm}"
                    if case.pair:
                        dw = _f32(ce.pair_weight(d["dw0"]))
                        cv.conv2d_pairs_wgrad(_bf(d["dy"]), _bf(ce.to_pairs(d["x"]), cl=False), 7, ce.STEM_S2, 2, dw, db)
                        torch.cuda.synchronize()
                        got = ce.unpair_weight(dw.cpu())
                    else:
                        dw = d["dw0"].float().cuda().contiguous(memory_format=CL)     # (K, R, S, C) storage
                        C_.conv_wgrad(_bf(d["dy"]), _bf(d["x"]), dw, db, _wg_geo(case))
                        torch.cuda.synchronize()
                        got = dw
                    _wg_compare(case, leg, what + " dw", got, dwr, Aw, "gauss_dw")
                    if bias:
                        _wg_compare(case, leg, what + " db", db, dbr, Ab, "gauss_db")
