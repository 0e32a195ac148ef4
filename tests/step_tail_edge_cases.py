"""Cases, data, fp64 / integer oracles and launch-geometry mirrors for the kernels that end a training step: the fused
log-softmax + NLL loss, the SGD / Adam / adaptive updates, sumsq / scale_f32, the fp32 <-> bf16 casts, the flat ReLU /
add helpers, the bf16 column sum and fill_bytes (csrc/elementwise.hip, csrc/optim.hip, f32_to_bf16_rtz of
csrc/nn_misc.hip). Pure torch: tests/test_step_tail_edges_cpu.py checks this file on its own,
tests/test_step_tail_edges_gpu.py holds the kernels to it.

Two kinds of reference:
* exact legs: data for which every fp32 intermediate is an fp32 number (``is_f32``), so a kernel equals the fp64
  oracle bit for bit whatever the order of its sums, its FMA contraction or its atomics;
* element-wise legs: Gaussian data against fp64 under a stated bound per element, or a distance in fp32 ulps.
"""
import math

import torch

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U24 = 2.0 ** -24

# ------------------------------------------------------------------------------------------------ launch geometry
DET_SLOTS = 128          # BIGDL_DET_SLOTS   (csrc/kernels.h)
XENT_SLOTS = 2048        # BIGDL_XENT_SLOTS
GRID_CAP = 8192          # grid_cap() default of csrc/elementwise.hip, the block cap of bigdl_optim_step
SUMSQ_CAP = 2048
FILL_CAP = 4096
COLSUM_CAP = 2048
RTZ_CAP = 16384          # blocks_for() of csrc/nn_misc.hip: the truncating cast's grid


def grid_cap(work, cap=GRID_CAP):
    return max(1, min(cap, (work + 255) // 256))


def past_cap(per_lane, cap=GRID_CAP, extra=0):
    """Smallest element count at which a 256-thread grid of ``cap`` blocks, ``per_lane`` elements per lane, takes a
    second grid-stride trip (+ ``extra`` elements of scalar tail)."""
    n = cap * 256 * per_lane + per_lane + extra
    assert grid_cap((n - extra) // per_lane, cap) == cap and (n - extra) // per_lane > cap * 256
    return n


SGD4_PAST_CAP = past_cap(4)              # 8192 x 256 x 4 + 4
SGD1_PAST_CAP = past_cap(1)              # 8192 x 256 + 1
CAST_PAST_CAP = past_cap(4, extra=1)     # 8192 x 256 x 4 + 5
RELU_PAST_CAP = past_cap(8, extra=3)     # 8192 x 256 x 8 + 11
SUMSQ_PAST_CAP = past_cap(1, SUMSQ_CAP)  # 2048 x 256 + 1
FILL_PAST_CAP = past_cap(16, FILL_CAP, extra=5)   # 4096 x 256 x 16 + 21
RTZ_PAST_CAP = past_cap(4, RTZ_CAP, extra=1)      # 16384 x 256 x 4 + 5: the truncating cast's second trip
OPTIM4_PAST_CAP = SGD4_PAST_CAP          # optim4_kernel: 4 elements per lane, 8192 blocks
XENT_PAST_CAP_ROWS = XENT_SLOTS * 4 + 5  # 8197 rows: one wave per row, 4 per block, 2048 blocks
assert (SGD4_PAST_CAP, SGD1_PAST_CAP, CAST_PAST_CAP) == (8192 * 256 * 4 + 4, 8192 * 256 + 1, 8192 * 256 * 4 + 5)
assert (RELU_PAST_CAP, SUMSQ_PAST_CAP, FILL_PAST_CAP) == (8192 * 256 * 8 + 11, 2048 * 256 + 1, 4096 * 256 * 16 + 21)


def xent_blocks(B):
    """Blocks of bigdl_softmax_xent through the binding (which passes a workspace whenever it has a loss, so the
    deterministic mode keeps the grid)."""
    return min((B + 3) // 4, XENT_SLOTS)


def xent_path(K, bf):
    """'vec' (16-byte loads) or 'scalar', and how many trips the busiest lane makes."""
    per = 8 if bf else 4
    vec = K % per == 0
    units = K // per if vec else K
    return ("vec" if vec else "scalar"), (units + 63) // 64


def colsum_grid(P, K, det):
    """(bx, by, rows per block) of bigdl_colsum_bf16_ld through the binding (deterministic: with its workspace)."""
    bx = (K // 8 + 63) // 64
    by = (P + 255) // 256
    if det:
        by = max(1, min(by, DET_SLOTS))
        rpb = (P + by - 1) // by
        return bx, (P + rpb - 1) // rpb, rpb
    if bx * by > COLSUM_CAP:
        by = (COLSUM_CAP + bx - 1) // bx
    by = max(by, 1)
    return bx, by, (P + by - 1) // by


def colsum_past_cap_case():
    """Smallest (P, K) at which the default column sum would ask for more than 2048 blocks and caps its row blocks."""
    best = None
    for K in (8, 520):                                   # one and two column blocks
        bx = (K // 8 + 63) // 64
        P = (COLSUM_CAP // bx) * 256 + 1
        assert bx * ((P + 255) // 256) > COLSUM_CAP >= bx * ((P - 1 + 255) // 256)
        if best is None or P * K < best[0] * best[1]:
            best = (P, K)
    return best


COLSUM_DET_PAST_SLOTS = (DET_SLOTS * 256 + 1, 24)       # more than DET_SLOTS row blocks of 256 rows


# ------------------------------------------------------------------------------------------------ comparisons
def gen(seed):
    return torch.Generator().manual_seed(seed)


def is_f32(t):
    """Every element of the fp64 tensor is an fp32 number."""
    return bool((t.to(F32).to(F64) == t).all())


def bits(t):
    t = t.detach().contiguous().cpu()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    """Bit equality (signed zeros and NaN payloads included)."""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def same_bits_nan(a, b):
    """Bit equality wherever ``b`` is a number; NaN exactly where ``b`` is NaN (any payload)."""
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    nb = torch.isnan(b)
    return torch.equal(torch.isnan(a), nb) and torch.equal(bits(a)[~nb], bits(b)[~nb])


def equals_f64(got, want64):
    """got (fp32 / bf16) == the fp64 oracle exactly, signed zero aside."""
    return torch.equal(got.detach().to(F64), want64.detach().to(F64).to(got.device))


def _pow2_floor(a):
    """2^floor(log2 a) of a positive fp64 tensor."""
    return torch.ldexp(torch.ones_like(a), torch.frexp(a)[1] - 1)


def ulp32(v):
    """Spacing of fp32 at |v| (fp64 tensor), the denormal spacing 2^-149 at the bottom."""
    a = v.abs().clamp_min(2.0 ** -126)
    return _pow2_floor(a) * 2.0 ** -23


def ulp_dist(got, want64, at=None, mag=None):
    """Largest |got - want| in fp32 ulps of the fp64 oracle value. ``at`` / ``mag``: further fp64 tensors; the ulp is
    then taken at the largest magnitude among the oracle value and them. For a difference of two terms
    (w - rate * d) the ulp is taken at the larger term, as profiles/bn_pool_edge_errors.txt does: the subtraction
    itself is one rounding of the result, but the error the subtrahend already carries does not shrink when the
    difference cancels."""
    want64 = want64.to(F64)
    ref = want64.abs()
    for t in list(at or ()) + ([] if mag is None else [mag]):
        ref = torch.maximum(ref, t.to(F64).abs().to(ref.device))
    d = (got.to(F64) - want64).abs() / ulp32(ref)
    return float(d.max()) if d.numel() else 0.0


def bf16_half_spacing(v):
    """Half the spacing of bf16 at |v| (fp64 tensor): the largest error of a correctly rounded bf16 store."""
    a = v.abs().clamp_min(2.0 ** -126)
    return _pow2_floor(a) * 2.0 ** -8


# ------------------------------------------------------------------------------------------------ canaries
SENTINEL = 0x5A
GUARD = 256              # bytes of sentinel on each side; keeps a view at offset 0 on a 256-byte boundary


def guarded(n, dtype, device, off=0):
    """(view of n elements, whole uint8 buffer, lead bytes): the view starts ``off`` elements past a 256-byte boundary
    inside a larger allocation filled with SENTINEL bytes."""
    es = torch.empty(0, dtype=dtype).element_size()
    lead = GUARD + off * es
    full = torch.full((lead + n * es + GUARD,), SENTINEL, dtype=torch.uint8, device=device)
    return full[lead:lead + n * es].view(dtype), full, lead


def canaries_ok(full, lead, nbytes):
    return bool((full[:lead] == SENTINEL).all()) and bool((full[lead + nbytes:] == SENTINEL).all())


# ================================================================================================== softmax + NLL
XENT_K = (1, 7, 8, 63, 64, 65, 72, 512, 520, 1000, 1003)
XENT_B = (1, 3, 4, 5)


def xent_oracle(logits, labels, label_base, scale):
    """fp64 loss (scalar), gradient [B, K], per-row losses and the mask of rows whose label lies in [0, K): a row
    outside is a skipped sample (ClassNLLCriterion's paddingValue): no loss, zero gradient row."""
    x = logits.to(F64)
    B, K = x.shape
    tgt = (labels.to(F64) - label_base).to(torch.int64)       # truncation towards zero, as the kernel's (int)
    valid = (tgt >= 0) & (tgt < K)
    lsm = torch.log_softmax(x, 1)
    t = tgt.clamp(0, K - 1)
    rows = torch.where(valid, -lsm.gather(1, t[:, None])[:, 0], torch.zeros_like(lsm[:, 0])) * scale
    onehot = torch.zeros_like(x).scatter_(1, t[:, None], 1.0)
    grad = torch.where(valid[:, None], (lsm.exp() - onehot) * scale, torch.zeros_like(x))
    return rows.sum(), grad, rows, valid


def xent_grad_bound(logits, grad64, scale, out_dtype):
    """Per-element bound of the gradient: 2^-24 (4 + |x - max|) p |scale| (the exponential's argument error grows with
    |x - max|; the sum, the reciprocal, the product and the scale are one rounding each), + the rounding of the result
    itself: for a bf16 result the half-spacing of bf16 at the exact value x (1 + 2^-6); for an fp32 result 2^-24 |g|
    (p - 1 at the target column and its product with the scale are two roundings of half an ulp of a value near
    |scale|, not near p |scale|: without this term the correctly rounded fp32 gradient fails at the target column)."""
    x = logits.to(F64)
    p = torch.softmax(x, 1)
    dist = (x - x.max(1, keepdim=True).values).abs()
    dist = torch.where(torch.isinf(dist), torch.zeros_like(dist), dist)      # a -inf logit: p == 0, bound 0
    # + the smallest normal fp32 x |scale|: exp() of sigma = 30 logits reaches the denormals, where the spacing no
    # longer shrinks with the value and the hardware exponential may flush its result to zero
    b = U24 * (4 + dist) * p * abs(scale) + 2.0 ** -126 * abs(scale)
    if out_dtype == BF:
        b = b + bf16_half_spacing(grad64) * (1 + 2.0 ** -6)
    else:
        b = b + U24 * grad64.abs()
    return b


def xent_grad_ratio(got, logits, grad64, scale):
    """Largest |got - exact| / bound (0 / 0 counts as 0: a zero gradient under a zero bound must be exactly zero)."""
    err = (got.to(F64) - grad64).abs()
    bound = xent_grad_bound(logits, grad64, scale, got.dtype)
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max())


def xent_loss_units(logits, labels, label_base, scale, blocks):
    """(reordering bound, per-row unit sum). Reordering: any order of adding B fp32 row losses (and `blocks` partials
    onto the pre-loaded loss) is within 2 (B - 1 + blocks) 2^-24 sum |row loss| of their sum
    (tests/test_det_reductions_gpu.py). Row unit: 2^-24 (4 + |max| + |lse| + |x_t|) |scale|, the roundings of
    max + log(sum) - x_t and the scale; the measured factor on it is in profiles/step_tail_edge_errors.txt."""
    x = logits.to(F64)
    _, _, rows, valid = xent_oracle(logits, labels, label_base, scale)
    B, K = x.shape
    t = (labels.to(F64) - label_base).to(torch.int64).clamp(0, K - 1)
    lse = torch.logsumexp(x, 1)
    unit = U24 * (4 + x.max(1).values.abs() + lse.abs() + x.gather(1, t[:, None])[:, 0].abs()) * abs(scale)
    unit = torch.where(valid, unit, torch.zeros_like(unit))
    reorder = 2 * max(B - 1 + blocks, 1) * U24 * 1.01 * float(rows.abs().sum())
    return reorder, float(unit.sum())


def xent_uniform(B, K, c=3.0):
    """Exact leg: all-equal logits, K a power of two: softmax == 1/K, exp(0) == 1 and K x (1/K) == 1 exactly."""
    assert K & (K - 1) == 0
    return torch.full((B, K), c)


def xent_spike(B, K, cols):
    """Exact leg: -200 everywhere, 0 at column cols[b]: exp(-200) underflows to 0 in fp32 (and adds 3e-85 relative in
    fp64, below half an ulp of 1), so lse == 0, p == onehot(col)."""
    x = torch.full((B, K), -200.0)
    x[torch.arange(B), torch.as_tensor(cols)] = 0.0
    return x


def xent_uniform_expect(K, labels, label_base, scale):
    """(1/K - onehot) * scale: every factor a power of two or an fp32 number, exact in fp32 and in fp64."""
    t = (labels.to(F64) - label_base).to(torch.int64)
    return (1.0 / K - torch.zeros(len(t), K, dtype=F64).scatter_(1, t[:, None], 1.0)) * scale


def xent_spike_expect(K, cols, labels, label_base, scale):
    """Spike rows: (per-row loss, gradient). Label on the spike: 0 and a zero row; label i elsewhere: 200 * scale,
    +scale at the spike, -scale at i."""
    t = (labels.to(F64) - label_base).to(torch.int64)
    cols = torch.as_tensor(cols)
    B = len(t)
    g = torch.zeros(B, K, dtype=F64)
    g[torch.arange(B), cols] += scale
    g[torch.arange(B), t] -= scale
    return torch.where(t == cols, 0.0, 200.0 * scale).to(F64), g


def granule_positions(K, per):
    """Columns worth pinning: every position of the first 16-byte granule, the last column, the scalar tail."""
    pos = set(range(min(per, K))) | {K - 1, K // 2}
    if K % per:
        pos |= set(range(K - K % per, K))
    if K > 64 * per:
        pos |= {64 * per, 64 * per + 1}                        # second trip of lane 0
    return sorted(pos)


def xent_gauss(B, K, sigma, offset, seed, dtype):
    x = torch.randn(B, K, generator=gen(seed)) * sigma + offset
    return x.to(dtype)


def xent_neg_inf_cases(K, per):
    """Column sets to set to -inf: first in lane 0's stride, last in it, a whole lane's stride, a middle column."""
    vec = K % per == 0
    step = per if vec else 1                                   # columns a lane takes per trip
    lane_cols = lambda lane: [c for c in range(K) if (c // step) % 64 == lane]   # noqa: E731
    l0 = lane_cols(0)
    out = {"first_of_lane0": [l0[0]], "last_of_lane0": [l0[-1]], "whole_lane1": lane_cols(1) or [K - 1]}
    if len(l0) > 1:
        out["all_but_last_of_lane0"] = l0[:-1]
    return {k: v for k, v in out.items() if 0 < len(v) < K}


# ================================================================================================== SGD
SGD_N = (1, 3, 4, 5, 1024, 1027)
# (lr, wd, momentum, dampening, nesterov): dyadic, exact in fp32 over three steps on integer data in [-8, 8]
SGD_EXACT_HP = (
    (0.5, 0.25, 0.5, 0.25, False),
    (0.5, 0.25, 0.5, 0.0, True),
    (0.5, 0.125, 0.75, 0.5, False),
    (0.5, 0.0, 0.5, 0.0, False),
    (0.5, 0.25, 0.0, 0.0, False),       # no momentum: mom untouched
    (0.25, 0.0, 0.0, 0.0, False),
)


def f32v(v):
    """The value a kernel sees when the binding narrows a Python float to fp32."""
    return float(torch.tensor(v, dtype=F32))


def int_vec(n, seed, lim=8):
    return torch.randint(-lim, lim + 1, (n,), generator=gen(seed)).to(F32)


def seg_decay_vector(seg_off, seg_wd, n, base):
    """Per-element extra decay of elements base .. base + n - 1: segment i covers [seg_off[i], seg_off[i + 1]); as in
    the kernels' search, the last segment starting at or before the element wins (a zero-length segment never does),
    and an element below seg_off[0] takes segment 0."""
    gi = base + torch.arange(n, dtype=torch.int64)
    idx = (torch.searchsorted(torch.as_tensor(seg_off, dtype=torch.int64), gi, right=True) - 1).clamp_min(0)
    return torch.as_tensor(seg_wd, dtype=F64)[idx]


def sgd_oracle(w, g, mom, lr, wd, momentum, dampening, nesterov, first, decay=None, track=None):
    """One step in fp64 from the given state (S/optim/SGD.scala:54-120). Returns (w, mom); mom is returned unchanged
    with momentum 0. ``track``: list that receives every intermediate (for the exactness check). The hyper-parameters
    are the doubles the method was given: narrowing them to fp32 is part of what the kernel is measured for."""
    w, g = w.to(F64), g.to(F64)
    dec = wd if decay is None else wd + decay.to(F64)
    t = [dec * w]
    d = g + t[-1]
    t.append(d)
    if momentum != 0:
        if first:
            b = d
        else:
            t += [momentum * mom.to(F64), (1 - dampening) * d]
            b = t[-2] + t[-1]
        t.append(b)
        mom = b
        if nesterov:
            t.append(momentum * b)
            d = d + t[-1]
            t.append(d)
        else:
            d = b
    t.append(lr * d)
    w = w - t[-1]
    t.append(w)
    if track is not None:
        track.extend(t)
    return w, mom


def mag_of(*terms):
    """Largest magnitude among the terms of a sum: where ``ulp_dist`` takes the ulp of a result that may cancel."""
    m = terms[0].to(F64).abs()
    for t in terms[1:]:
        m = torch.maximum(m, t.to(F64).abs())
    return m


def sgd_mags(w, g, mom, lr, wd, momentum, dampening, nesterov, first):
    """Magnitudes for the ulp distances of one Gaussian-data step: mom = momentum mom + (1 - dampening) (g + wd w) and
    w - lr d are sums that can cancel; each is measured at its largest term."""
    w, g = w.to(F64), g.to(F64)
    d_terms = [g, wd * w]
    if momentum == 0:
        return {"w": mag_of(w, *(lr * t for t in d_terms)), "mom": None}
    b_terms = d_terms if first else [momentum * mom.to(F64)] + [(1 - dampening) * t for t in d_terms]
    step = [lr * t for t in b_terms]
    if nesterov:
        step = [lr * momentum * t for t in b_terms] + [lr * t for t in d_terms]
    return {"w": mag_of(w, *step), "mom": mag_of(*b_terms)}


def sgd_exact_run(n, hp, seed, steps=3, decay=None):
    """Three exact steps on integer data: list of (g, w_after, mom_after) in fp64, the start w, and whether every
    intermediate was an fp32 number."""
    lr, wd, momentum, dampening, nesterov = hp
    w0 = int_vec(n, seed)
    w, mom, out, track = w0.to(F64), torch.zeros(n, dtype=F64), [], []
    for s in range(steps):
        g = int_vec(n, seed + 100 + s)
        w, mom = sgd_oracle(w, g, mom, lr, wd, momentum, dampening, nesterov, s == 0, decay, track)
        out.append((g, w, mom))
    return w0, out, all(is_f32(t) for t in track)


# segment layouts: (seg_off, seg_wd, base, n): boundaries at every position inside a group of four, a zero-length
# segment, a range that starts inside a segment (the ZeRO shard case)
def seg_cases():
    nine_off = [0, 5, 6, 7, 8, 8, 13, 22, 31]          # boundaries at residues 1, 2, 3, 0 (zero-length at 8), 1, 2, 3
    nine_wd = [0.25, 0.0, 0.5, 0.125, 1.0, 0.25, 0.0, 0.375, 0.5]
    return {
        "one": ([0], [0.25], 0, 37),
        "two": ([0, 18], [0.0, 0.5], 0, 37),
        "two_b1": ([0, 17], [0.25, 0.125], 0, 36),
        "two_b3": ([0, 19], [0.25, 0.125], 0, 36),
        "nine": (nine_off, nine_wd, 0, 40),
        "nine_scalar": (nine_off, nine_wd, 0, 39),
        "shard": ([0, 10, 50, 61, 200], [0.5, 0.25, 0.0, 0.125, 1.0], 24, 64),       # starts inside segment 1
        "shard_odd": ([0, 10, 50, 61, 200], [0.5, 0.25, 0.0, 0.125, 1.0], 27, 35),
        "shard_tail": ([0, 10, 50], [0.5, 0.25, 0.125], 52, 16),                     # wholly inside the last segment
    }


# ================================================================================================== Adam / adaptive
ADAM_N = (1, 3, 4, 5, 1027)
ADAM_PAST_CAP = SGD1_PAST_CAP


def adam_oracle(w, g, m, v, lr, b1, b2, eps, wd, t):
    """BigDL Adam (S/optim/Adam.scala:36) in fp64 on the doubles the method holds; bc1 / bc2 as optim/methods.py
    computes them."""
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    w, g, m, v = (x.to(F64) for x in (w, g, m, v))
    gi = g + wd * w
    mag = {"m": mag_of(b1 * m, (1 - b1) * g, (1 - b1) * wd * w)}
    mag["v"] = mag_of(b2 * v, (1 - b2) * gi * mag_of(g, wd * w))      # gi^2 carries twice the error of a cancelled gi
    m = b1 * m + (1 - b1) * gi
    v = b2 * v + (1 - b2) * gi * gi
    k = lr * (math.sqrt(bc2) / bc1) / (v.sqrt() + eps)
    mag["w"] = mag_of(w, k * mag["m"])          # the step inherits m's error at m's largest term
    w = w - k * m
    return w, m, v, mag


# method id, name, hyper-parameters (a .. e of OptimHP), has a second state tensor, start value of s1
OPTIM_METHODS = (
    (0, "adagrad", (0.1, 1e-3, 0.0, 0.0, 0.0), False, 0.0),
    (1, "rmsprop", (0.01, 0.9, 1e-6, 0.0, 0.0), False, 0.0),
    (2, "adadelta", (0.9, 1e-6, 0.0, 0.0, 0.0), True, 0.0),
    (3, "adamax", (0.02 / (1 - 0.9), 0.9, 0.999, 1e-38, 0.0), True, 0.0),
    (4, "ftrl", (0.1, -0.5, 0.01, 0.02, 0.03), True, 0.1),
    (4, "ftrl_pow", (0.1, -0.6, 0.01, 0.02, 0.0), True, 0.1),       # the general-power branch, measured separately
)


def optim_oracle(method, hp, x, g, s1, s2):
    """update1 of csrc/optim.hip in fp64 on the doubles the method holds. Returns (x, s1, s2, mag): mag[name] is the
    magnitude at which the ulp of that output is taken (the largest term of the sums that can cancel; ``mag_of``)."""
    a, b, c, d, e = hp
    x, g, s1 = x.to(F64), g.to(F64), s1.to(F64)
    s2 = None if s2 is None else s2.to(F64)
    mag = {}
    if method == 0:
        g0 = g
        g = g + b * x
        mag["s1"] = mag_of(s1, g * mag_of(g0, b * x))       # g^2 carries twice the error of a cancelled g + wd x
        s1 = s1 + g * g
        k = a / (s1.sqrt() + 1e-10)
        mag["x"] = mag_of(x, k * g0, k * b * x)
        x = x - k * g
    elif method == 1:
        s1 = b * s1 + (1 - b) * g * g
        mag["x"] = mag_of(x, a * g / (s1.sqrt() + c))
        x = x - a * g / (s1.sqrt() + c)
    elif method == 2:
        s1 = a * s1 + (1 - a) * g * g
        dl = (s2 + b).sqrt() / (s1 + b).sqrt() * g
        mag["x"] = mag_of(x, dl)
        x = x - dl
        s2 = a * s2 + (1 - a) * dl * dl
    elif method == 3:
        mag["s1"] = mag_of(b * s1, (1 - b) * g)
        s1 = b * s1 + (1 - b) * g
        s2 = torch.maximum(c * s2, g.abs() + d)
        mag["x"] = mag_of(x, a * mag["s1"] / s2)
        x = x - a * s1 / s2
    elif method == 4:
        gs = g + 2 * e * x if e > 0 else g
        acc = s1 + g * g
        if b == -0.5:
            r0, r1 = s1.sqrt(), acc.sqrt()
        else:
            r0, r1 = s1.pow(-b), acc.pow(-b)
        sigma, quad = (r1 - r0) / a, r1 / a + 2 * d
        # sigma = (r1 - r0) / a cancels: its error is that of r1 / a, and sigma x carries it into s2 and on into x
        mag["s2"] = mag_of(s2, g, 2 * e * x, r1 / a * x)
        s2 = s2 + gs - sigma * x
        l1 = torch.sign(s2) * c
        # the soft threshold is continuous ((l1 - s2) / quad is 0 at |s2| == l1): an element that falls on the other
        # side of it in fp32 is off by no more than s2's own error over quad, which mag["x"] covers
        mag["x"] = mag_of((l1 - s2) / quad, mag["s2"] / quad)
        x = torch.where(s2.abs() > c, (l1 - s2) / quad, torch.zeros_like(x))
        s1 = acc
    else:
        raise ValueError(method)
    return x, s1, s2, mag


# ================================================================================================== sumsq / scale
SUMSQ_N = (1, 255, 256, 257)


def sumsq_oracle(x, start=0.0):
    return float((x.to(F64) ** 2).sum()) + start


def sumsq_chain(n, mode):
    """Roundings on the longest chain from an element to ``out``: the lane's running sum (+ one for each square), the
    6 shuffle steps, 3 wave adds, then the blocks' atomics in any order (default), the ordered 128 slots
    (deterministic with workspace) or one block's atomic, + the add onto the pre-loaded out."""
    blocks = {"default": grid_cap(n, SUMSQ_CAP), "det_ws": DET_SLOTS, "det_one": 1}[mode]
    per_lane = (n + blocks * 256 - 1) // (blocks * 256)
    return per_lane + 1 + 6 + 3 + blocks + 1


def sumsq_bound(x, start, mode):
    return U24 * sumsq_chain(x.numel(), mode) * (float((x.to(F64) ** 2).sum()) + abs(start))


# ================================================================================================== casts
def cast_edge_bits():
    """fp32 bit patterns at the rounding edges of bf16 (positive; the table also carries their negatives)."""
    pos = [
        0x3F808000,   # tie, kept mantissa even  -> down
        0x3F818000,   # tie, kept mantissa odd   -> up
        0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001,      # one ulp either side of both ties
        0x3F80FFFF,   # just under the next bf16
        0x7F7FFFFF,   # largest finite: inf under nearest-even, largest bf16 under truncation
        0x7F7F7FFF, 0x7F7F8000,                              # below / at the last tie before inf
        0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x007FFFFF, 0x00800000,   # denormals, smallest normal
        0x00000000, 0x7F800000,                              # zero, inf
        0x3F800000, 0x40490FDB,
    ]
    nan = [0x7FC00000, 0x7F800001, 0x7F80FFFF, 0x7FFFFFFF, 0x7F810000]   # two with the payload only in the low 16 bits
    allb = pos + [b | 0x80000000 for b in pos] + nan + [b | 0x80000000 for b in nan]
    return torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in allb], dtype=torch.int32)


def cast_input(n, seed):
    """n fp32 values: the edge table repeated through every n % 4 residue (each repeat shifted by one slot), Gaussian
    filler, and the table again at the very end so it also lands in the scalar tail."""
    tab = cast_edge_bits().view(F32)
    x = torch.randn(n, generator=gen(seed)) * 3
    if n >= 4 * (tab.numel() + 4):
        pos = 0
        for r in range(4):
            x[pos + r:pos + r + tab.numel()] = tab
            pos += tab.numel() + 4 - (tab.numel() % 4)
    m = min(n, tab.numel())
    x[n - m:] = tab[:m] if n < tab.numel() else tab
    if n <= 5:
        x[:] = tab[[1, 7, 12, 20 + 1, 40][:n]]
    return x


def rne_oracle(x):
    return x.to(BF)


def rtz_oracle(x):
    """The CPU f32_to_bf16_rtz (ops/nnk.py): the upper 16 bits. Pinned consequences: the largest finite fp32 becomes the
    largest finite bf16; a NaN whose payload lies only in the low 16 bits (0x7F800001) becomes +-inf (0x7F80)."""
    return (x.contiguous().view(torch.int32) >> 16).to(torch.int16).view(BF)


# ================================================================================================== relu / add
RELU_N = (1, 7, 8, 9, 15, 1001)


def bf16_special():
    return torch.tensor([0.0, -0.0, float("inf"), -float("inf"), float("nan"), -float("nan"), 2.0 ** -130, -2.0 ** -130,
                         2.0 ** -133, 1.0, -1.0, 3.3895e38, -3.3895e38, 0.5, -2.0 ** -126, 2.0 ** -126]).to(BF)


def bf16_input(n, seed):
    """Gaussian bf16 with the special values spread over every n % 8 residue, and in the tail."""
    x = (torch.randn(n, generator=gen(seed)) * 2).to(BF)
    sp = bf16_special()
    idx = torch.randperm(n, generator=gen(seed + 1))[:min(n, 3 * sp.numel())]
    x[idx] = sp.repeat(3)[:idx.numel()]
    m = min(n, 7)
    x[n - m:] = sp[torch.randperm(sp.numel(), generator=gen(seed + 2))[:m]]
    return x


def relu_fwd_oracle(x):
    """Threshold(0, 0) of the reference (S/nn/Threshold.scala:83: x <= th ? v : x): +0 for x <= 0 (-0 included), x's
    own bits otherwise, so a NaN passes with its payload, as torch.relu propagates it."""
    return torch.where(x.float() <= 0, torch.zeros_like(x), x)


def relu_bwd_oracle(dy, y):
    """dy's own bits where y > 0 (a NaN dy included), +0 elsewhere (a NaN y included: y > 0 is false)."""
    return torch.where(y.float() > 0, dy, torch.zeros_like(dy))


def add_oracle(a, b):
    return (a.float() + b.float()).to(BF)


# ================================================================================================== colsum / fill
COLSUM_K = (8, 24, 512, 520)
COLSUM_P = (1, 3, 4, 5, 255, 256, 257)


def int_rows_bf16(P, K, seed, lim=4, device="cpu"):
    """Integers in [-lim, lim]: column sums of up to 2^24 / lim rows are exact in fp32 in any order."""
    assert P * lim < 2 ** 24
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randint(-lim, lim + 1, (P, K), generator=g, device=device, dtype=torch.int8).to(BF)


def colsum_oracle(x, start):
    return x.to(F64).sum(0) + start.to(F64)


FILL_BYTES = (1, 15, 16, 17)
