"""Deterministic-mode reductions on the Transformer path: the embedding gradient (csrc/nn_misc.hip,
embedding_bwd_sorted_kernel) bit for bit against a CPU emulation of its stated order, and LayerNorm's parameter
gradients (csrc/layernorm.hip: per-chunk partials, summed in chunk order) bitwise run to run and against fp64, and the
cross-entropy loss (csrc/elementwise.hip: per-block partials on the full grid, added in a fixed order).
Every test restores the mode it found."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

from tests.test_det_routes_cpu import embedding_emulation

pytestmark = pytest.mark.gpu

EPS = 1e-6


@contextlib.contextmanager
def _mode(det):
    from bigdl_amd.ops import native

    saved = native.deterministic()
    native.get()
    native.set_deterministic(det)
    try:
        yield native.get()
    finally:
        native.set_deterministic(saved)


# ------------------------------------------------------------------------------------------------ embedding
N_POS, N_ROWS, D_EMB = 4096, 50, 70
LIVE_ROWS = (3, 7, 8, 20, 21, 33, 49)                    # 0-based weight rows that receive gradient
PAD_ROW = 12                                             # 0-based row named as pad: present in the ids, skipped


def _embedding_data():
    g = torch.Generator().manual_seed(70)
    rows = torch.tensor(LIVE_ROWS)[torch.randint(0, len(LIVE_ROWS), (N_POS,), generator=g)]
    gout = torch.randn(N_POS, D_EMB, generator=g)
    gw0 = torch.randn(N_ROWS, D_EMB, generator=g)        # non-zero starting gradient
    special = torch.randperm(N_POS, generator=g)
    return rows, gout, gw0, special[:300], special[300:500]


@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_embedding_bwd_bit_for_bit(scale):
    rows, gout, gw0, skip, _ = _embedding_data()
    idx = rows.clone()
    idx[skip] = -1
    want = embedding_emulation(gout, idx, gw0, scale)
    gw = gw0.clone().cuda()
    with _mode(True) as C:
        C.embedding_bwd(gout.cuda(), idx.cuda(), gw, scale)
        torch.cuda.synchronize()
    assert torch.equal(gw.cpu(), want)
    untouched = [r for r in range(N_ROWS) if r not in LIVE_ROWS]
    assert torch.equal(gw.cpu()[untouched], gw0[untouched])


@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16], ids=["gf32", "gbf16"])
@pytest.mark.parametrize("idt", [torch.float32, torch.int64], ids=["idf32", "idi64"])
def test_embedding_bwd_ids_bit_for_bit(idt, gdt, scale):
    rows, gout, gw0, zero, pad = _embedding_data()
    ids = rows + 1                                       # raw 1-based ids
    ids[zero] = 0                                        # masked
    ids[pad] = PAD_ROW + 1                               # the pad id: skipped
    keys = ids - 1
    keys[keys == PAD_ROW] = -1
    g_dev = gout.to(gdt)
    want = embedding_emulation(g_dev.float(), keys, gw0, scale)
    gw = gw0.clone().cuda()
    with _mode(True) as C:
        C.embedding_bwd_ids(g_dev.cuda(), ids.to(idt).cuda(), gw, PAD_ROW, scale)
        torch.cuda.synchronize()
    assert torch.equal(gw.cpu(), want)
    untouched = [r for r in range(N_ROWS) if r not in LIVE_ROWS]
    assert PAD_ROW in untouched
    assert torch.equal(gw.cpu()[untouched], gw0[untouched])


@pytest.mark.parametrize("det", [False, True], ids=["default", "deterministic"])
def test_embedding_within_fp32_of_fp64(det):
    """Any summation order of n fp32 terms onto a start value is within (n + 1) 2^-24 (|start| + sum |terms|) of the
    exact sum (first-order bound of recursive summation, one more rounding for scale * g)."""
    rows, gout, gw0, skip, _ = _embedding_data()
    idx = rows.clone()
    idx[skip] = -1
    keep = idx >= 0
    scale = 0.75
    exact = gw0.double().index_add(0, idx[keep], gout[keep].double() * scale)
    mag = gw0.double().abs().index_add(0, idx[keep], gout[keep].double().abs() * scale)
    n = torch.bincount(idx[keep], minlength=N_ROWS).max().item()
    gw = gw0.clone().cuda()
    with _mode(det) as C:
        C.embedding_bwd(gout.cuda(), idx.cuda(), gw, scale)
        torch.cuda.synchronize()
    err = (gw.cpu().double() - exact).abs()
    assert (err <= (n + 2) * 2.0 ** -24 * mag).all(), err.max().item()


# ------------------------------------------------------------------------------------------------ loss
@pytest.mark.parametrize("B,K", [(3, 7), (8200, 104)])
def test_softmax_xent_loss_in_fixed_order_on_the_full_grid(B, K):
    """Deterministic mode keeps the default grid of the fused log-softmax + NLL kernel (8200 rows: past the
    2048-block cap, rows grid-strided) and adds the blocks' loss partials in a fixed order: the loss repeats bit for
    bit, the gradient is the default mode's bit for bit (rows are independent), and the loss is within the
    reordering bound of the default mode's, 2 (B - 1) 2^-24 sum |row loss| (both add the same fp32 row losses)."""
    g = torch.Generator().manual_seed(B)
    logits = (torch.randn(B, K, generator=g) * 3).cuda()
    labels = torch.randint(1, K + 1, (B,), generator=g).float().cuda()
    out = {}
    for det in (True, False):
        with _mode(det) as C:
            runs = []
            for _ in range(2):
                loss, d = torch.zeros(1, device="cuda"), torch.empty_like(logits)
                C.softmax_xent(logits, labels, loss, d, 1.0, 1.0)
                runs.append((loss, d))
            torch.cuda.synchronize()
        out[det] = runs
    assert torch.equal(out[True][0][0], out[True][1][0]) and torch.equal(out[True][0][1], out[True][1][1])
    assert torch.equal(out[True][0][1], out[False][0][1])
    rows = (torch.logsumexp(logits.double(), 1) - logits.double().gather(1, (labels.long() - 1)[:, None])[:, 0])
    bound = 2 * max(B - 1, 1) * 2.0 ** -24 * 1.01 * rows.abs().sum().item()
    assert abs(out[True][0][0].item() - out[False][0][0].item()) <= bound
    assert torch.isfinite(out[True][0][0]).all() and out[True][0][0].item() > 0


# ------------------------------------------------------------------------------------------------ LayerNorm
def _past_cap(D):
    """The smallest row count whose 64-row chunks exceed the 2048-block cap at this D, plus one partial chunk."""
    bx = (D + 255) // 256
    rows = (2048 // bx) * 64 + 65
    assert bx * ((rows + 63) // 64) > 2048
    return rows


def _ln_data(rows, D):
    gen = torch.Generator().manual_seed(rows * 8191 + D)
    x = torch.randn(rows, D, generator=gen) * 3 + 1
    dy = torch.randn(rows, D, generator=gen)
    g = torch.randn(D, generator=gen)
    b = torch.randn(D, generator=gen)
    return x, g, b, dy


def _cpu_param_grads(x, g, b, dy, dtype):
    """dgamma, dbeta of F.layer_norm by autograd on the CPU in ``dtype`` (the yardstick of
    tests/test_layernorm_edges_gpu.py)."""
    gs, bs = g.to(dtype).requires_grad_(True), b.to(dtype).requires_grad_(True)
    F.layer_norm(x.to(dtype), (x.shape[-1],), gs, bs, EPS).backward(dy.to(dtype))
    return gs.grad, bs.grad


def _native_param_grads(C, x, g, dy, dg, db):
    rows = x.shape[0]
    y, mean, rstd = torch.empty_like(x), x.new_empty(rows), x.new_empty(rows)
    C.layernorm_fwd(x, g, None, y, mean, rstd, EPS)
    C.layernorm_bwd(dy, x, g, mean, rstd, None, dg, db)
    return mean, rstd


@pytest.mark.parametrize("rows", [1, 65, 200, "cap"])
@pytest.mark.parametrize("D", [1, 70, 256, 257, 4096])
def test_layernorm_parameter_gradients(rows, D):
    """Bitwise equal across two calls, within the dgamma / dbeta bound of tests/test_layernorm_edges_gpu.py against
    fp64, and accumulating. That bound: the yardstick is the error of fp32 CPU F.layer_norm (forward and autograd)
    against fp64 on the same inputs, per tensor, and the kernel is held to |kernel - fp64| <= 4 x that + 1e-7
    max|fp64|: the kernel's column sums are fp32 sums of the same terms in another order, so its error is of the
    size of the CPU's own. Not to be widened."""
    rows = _past_cap(D) if rows == "cap" else rows
    x, g, b, dy = _ln_data(rows, D)
    xd, gd, dyd = x.cuda(), g.cuda(), dy.cuda()
    runs = []
    with _mode(True) as C:
        for _ in range(2):
            dg, db = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
            mean, rstd = _native_param_grads(C, xd, gd, dyd, dg, db)
            runs.append((dg, db))
        acc_g, acc_b = runs[1][0].clone(), runs[1][1].clone()
        C.layernorm_bwd(dyd, xd, gd, mean, rstd, None, acc_g, acc_b)      # once more into the same buffers
        torch.cuda.synchronize()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    hi = _cpu_param_grads(x, g, b, dy, torch.float64)
    lo = _cpu_param_grads(x, g, b, dy, torch.float32)
    for name, got, h, l in zip(("dg", "db"), runs[0], hi, lo):
        yard = (l.double() - h).abs().max().item()
        err = (got.cpu().double() - h).abs()
        bound = 4 * yard + 1e-7 * h.abs().max().item()
        worst = err.max().item()
        print(f"DET_RATIO layernorm {rows}x{D} {name} err={worst:.3e} yard={yard:.3e} "
              f"ratio={worst / yard if yard > 0 else float(worst > 0):.3f}")
        assert (err <= bound).all(), (name, worst, bound)
    # accumulate semantics: total + total is exact, so twice the single call within one rounding
    for acc, (single) in zip((acc_g, acc_b), runs[0]):
        twice = 2 * single.double()
        assert ((acc.double() - twice).abs() <= 2.0 ** -23 * twice.abs()).all()


@pytest.mark.parametrize("has_g,has_b", [(True, False), (False, True)])
def test_layernorm_gamma_or_beta_absent(has_g, has_b):
    rows, D = 200, 257
    x, g, b, dy = _ln_data(rows, D)
    xd, gd, dyd = x.cuda(), g.cuda(), dy.cuda()
    with _mode(True) as C:
        dg, db = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
        _native_param_grads(C, xd, gd, dyd, dg, db)
        one = torch.zeros(D, device="cuda")
        _native_param_grads(C, xd, gd if has_g else None, dyd, one if has_g else None, one if has_b else None)
        torch.cuda.synchronize()
    assert torch.equal(one, dg if has_g else db)


def test_layernorm_autograd_route_is_repeatable():
    """ops.norm.layer_norm in deterministic mode: parameter gradients bitwise equal across two backward passes."""
    from bigdl_amd.ops.norm import layer_norm

    x, g, b, dy = _ln_data(_past_cap(257), 257)
    grads = []
    with _mode(True):
        for _ in range(2):
            gl, bl = g.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
            layer_norm(x.cuda(), gl, bl, EPS).backward(dy.cuda())
            grads.append((gl.grad, bl.grad))
        torch.cuda.synchronize()
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
