"""The sum of the weight-gradient split partials (csrc/split_reduce.hip), driven through conv_wgrad with shapes whose
plan splits the pixels on every route: 1 x 1 / stride 1 and stride 2 (128 x 128 LDS-DMA kernel + workspace), 3 x 3 on
the halo kernel with the bias gradient folded into the same reduce launch, a weight whose float4 column count is no
multiple of the workgroup's columns, and dW as a 4-byte-aligned view of a flat buffer.

Per case: dW (and dbias) accumulate onto a known non-zero pattern and must equal pattern + the fp64 CPU reference of the
same bf16 inputs within twice the largest error measured at the parent commit on the same inputs (ERR_PARENT below,
profiles/wgrad_reduce_errors.txt: a fixed-order sum is no worse than the atomic order it replaces), and two calls on
the same inputs must give the same bits (the small 1 x 1 weights met in dW through fp32 atomics before)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

CL = torch.channels_last
BF = torch.bfloat16

# name -> (N, C, H, K, R, stride, pad, bias, dW offset in floats). N is the smallest batch to try: _case() raises it
# until the plan reports >= 3 workspace splits.
CASES = {
    "1x1_s1": (8, 64, 16, 64, 1, 1, 0, False, 0),          # n4 = 1024: the narrowest workgroup columns
    "1x1_s2": (8, 64, 16, 128, 1, 2, 0, False, 0),
    "3x3_halo_bias": (8, 64, 14, 64, 3, 1, 1, True, 0),    # 56 row-stage splits, bias partials behind the dW partials
    "awkward_columns": (8, 264, 16, 264, 1, 1, 0, False, 0),   # n4 = 17424 = 16 * 1089: a partial last workgroup
    "unaligned_dw": (8, 64, 16, 128, 1, 1, 0, False, 1),
}

# Largest error of the parent commit on these inputs (three runs each, all equal: at these split counts its reduce ran
# without atomics), in the measure of _errors(): max |got - (pattern + ref)| / max |ref|, (dW, dbias). The bound is
# twice that. This kernel measured 1.797e-07, 2.316e-07, 1.413e-07 / 5.276e-08, 2.250e-07 and 1.842e-07.
ERR_PARENT = {
    "1x1_s1": (1.7969e-07, None),
    "1x1_s2": (2.3163e-07, None),
    "3x3_halo_bias": (1.5340e-07, 5.2757e-08),
    "awkward_columns": (2.2498e-07, None),
    "unaligned_dw": (1.7351e-07, None),
}


def _C():
    from bigdl_amd.ops import native

    return native.get()


def _geo(N, C, H, K, R, st, pd):
    OH = (H + 2 * pd - R) // st + 1
    return [N, H, H, C, OH, OH, R, R, st, st, pd, pd, 1, 1, N * OH * OH, K, R * R * C, K], OH


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs (bf16, CPU), the fp64 reference of dW in (K, R, S, C) order and of dbias, and the plan: computed once."""
    N, C, H, K, R, st, pd, bias, offset = CASES[name]
    while True:
        geo, OH = _geo(N, C, H, K, R, st, pd)
        splits, wsn, halo, p8, reg = _C().conv_wgrad_plan_info(geo, bias)
        if splits >= 3 and wsn > 0:
            break
        N += 1
        assert N <= 64, f"{name}: no batch up to 64 splits the pixels three ways"
    gen = torch.Generator().manual_seed(4242)
    x = torch.randn(N, C, H, H, generator=gen).to(BF)
    dy = torch.randn(N, K, OH, OH, generator=gen).to(BF)
    ref = torch.nn.grad.conv2d_weight(x.double(), (K, C, R, R), dy.double(), stride=st, padding=pd)
    ref = ref.permute(0, 2, 3, 1).reshape(-1).contiguous()
    refb = dy.double().sum(dim=(0, 2, 3)) if bias else None
    return dict(geo=geo, x=x, dy=dy, ref=ref, refb=refb, splits=splits, halo=halo, bias=bias, offset=offset, K=K)


def _pattern(n):
    """A non-zero pattern of exact eighths in [-0.625, 0.875]."""
    return ((torch.arange(n) % 7).float() - 3.0) * 0.25 + 0.125


def _run(name):
    """One conv_wgrad call onto the pattern: (flat buffer, dW view, dbias)."""
    c = _case(name)
    dev = torch.device("cuda:0")
    x = c["x"].to(dev).contiguous(memory_format=CL)
    dy = c["dy"].to(dev).contiguous(memory_format=CL)
    n, off = c["ref"].numel(), c["offset"]
    flat = _pattern(n + off).to(dev)
    dw = flat[off:]
    db = _pattern(c["K"]).to(dev) if c["bias"] else None
    _C().conv_wgrad(dy, x, dw, db, c["geo"])
    torch.cuda.synchronize()
    return flat, dw, db


def _errors(name):
    """max |got - (pattern + ref)| / max |ref| of dW and of dbias (None without bias)."""
    c = _case(name)
    flat, dw, db = _run(name)
    off = c["offset"]
    assert torch.equal(flat[:off].cpu(), _pattern(off)), "the floats in front of the dW view were written"
    want = _pattern(c["ref"].numel() + off)[off:].double() + c["ref"]
    e_dw = ((dw.cpu().double() - want).abs().max() / c["ref"].abs().max()).item()
    e_db = None
    if c["bias"]:
        wantb = _pattern(c["K"]).double() + c["refb"]
        e_db = ((db.cpu().double() - wantb).abs().max() / c["refb"].abs().max()).item()
    return e_dw, e_db


def test_plans_split_on_every_route():
    for name in CASES:
        c = _case(name)
        assert c["splits"] >= 3, (name, c["splits"])
        assert (c["halo"] > 0) == (name == "3x3_halo_bias"), (name, c["halo"])
    # 264 x 264 / 4 float4 columns: no multiple of the 32 or 64 columns a workgroup owns at this size
    n4 = _case("awkward_columns")["ref"].numel() // 4
    assert n4 >= 16384 and n4 % 32 != 0
    assert _case("unaligned_dw")["offset"] % 4 != 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_accumulates_reference_onto_pattern(name):
    e_dw, e_db = _errors(name)
    p_dw, p_db = ERR_PARENT[name]
    print(f"{name}: dW error {e_dw:.3e} (parent {p_dw:.3e}, bound {2 * p_dw:.3e})"
          + (f", dbias error {e_db:.3e} (parent {p_db:.3e}, bound {2 * p_db:.3e})" if e_db is not None else ""))
    assert e_dw <= 2 * p_dw
    if e_db is not None:
        assert e_db <= 2 * p_db


@pytest.mark.parametrize("name", sorted(CASES))
def test_two_calls_are_bit_identical(name):
    _, dw1, db1 = _run(name)
    _, dw2, db2 = _run(name)
    assert torch.equal(dw1, dw2), "dW differs between two calls on the same inputs"
    if db1 is not None:
        assert torch.equal(db1, db2), "dbias differs between two calls on the same inputs"
