"""Cases, data and fp64 oracles for fused LARS (csrc/lars.hip, bigdl_amd/ops/lars.py). Pure torch and written without
ops/lars.py: tests/test_lars_cpu.py ties the oracle to the torch route of LarsProcessor + LarsSGD and checks the plan
builder's tables against it, tests/test_lars_gpu.py holds the kernels and the routes to it.

    nw = sqrt(sum w^2), ng = sqrt(sum g^2)              over the whole layer
    scale = (ng + WD nw) / nw;  inf -> 1e4, |scale| < 1e-4 -> 1e-4, nan -> 1     (this order)
    rate = rate_num / scale;  v = momentum v + (g + wd w) rate;  w -= v;  w16 = bf16(w)

* exact legs: integer patterns whose per-layer sums of squares are powers of 4, WD in {0, 1, 3}, dyadic
  hyper-parameters: every intermediate of three steps is an fp32 number, so the expectation is equality;
* Gaussian legs: the norms against a worst-case chain bound of the kernels' own summation order, the update in fp32
  ulps of the term magnitudes.
"""
import torch

from tests.step_tail_edge_cases import (F32, F64, U24, canaries_ok, gen, guarded, int_vec, is_f32, mag_of,  # noqa: F401
                                        same_bits, same_bits_nan, ulp_dist)

CHUNK = 4096             # BIGDL_LARS_CHUNK     (csrc/kernels.h)
BLOCK_CAP = 2048         # BIGDL_LARS_BLOCK_CAP
C = CHUNK

# piece lengths: below / at / above a 16-byte group, around one chunk, several chunks with a tail
LENGTHS = (1, 3, 4, 5, C - 1, C, C + 1, 2 * C + 3)
FINISH_SECOND_TRIP = 65 * C + 1          # 66 chunks: lane 0 of the finish wave adds partials 0, 64; lane 1 adds 1, 65
PAST_CAP_LENGTHS = (700 * C + 5, 700 * C + 1, 649 * C + 2)     # 2052 chunks > BLOCK_CAP: a second grid-stride trip
assert sum((n + C - 1) // C for n in PAST_CAP_LENGTHS) > BLOCK_CAP


def layout(lengths, base=0):
    """Consecutive pieces [(lo, hi, layer)], one layer each, the first at element ``base``; and the buffer length."""
    out, lo = [], base
    for i, n in enumerate(lengths):
        out.append((lo, lo + n, i))
        lo += n
    return out, lo


def split_two(pieces, cuts):
    """Two ranks' pieces: [0, cuts[0]) is rank A's, [cuts[0], cuts[1]) rank B's, and so on alternating; layer ids are
    kept, so a layer cut in two is one piece on each side."""
    edges = [0] + list(cuts) + [max(p[1] for p in pieces)]
    sides = ([], [])
    for k in range(len(edges) - 1):
        a, b = edges[k], edges[k + 1]
        for lo, hi, layer in pieces:
            x, y = max(a, lo), min(b, hi)
            if y > x:
                sides[k % 2].append((x, y, layer))
    return sides


# ------------------------------------------------------------------------------------------------ oracles (fp64)
def sums_oracle(w, g, pieces, nlayers):
    """acc[2 l], acc[2 l + 1] = sum w^2, sum g^2 over the pieces of layer l."""
    acc = torch.zeros(2 * nlayers, dtype=F64)
    w, g = w.to(F64), g.to(F64)
    for lo, hi, layer in pieces:
        acc[2 * layer] += (w[lo:hi] ** 2).sum()
        acc[2 * layer + 1] += (g[lo:hi] ** 2).sum()
    return acc


def scale_oracle(acc, WD):
    """Per-layer gradient scale with the guards in the order of LarsProcessor.collectGlobalData."""
    acc = acc.to(F64)
    nw, ng = acc[0::2].sqrt(), acc[1::2].sqrt()
    scale = (ng + WD * nw) / nw
    scale = torch.where(torch.isinf(scale), torch.full_like(scale, 1e4), scale)
    scale = torch.where(scale.abs() < 1e-4, torch.full_like(scale, 1e-4), scale)
    scale = torch.where(torch.isnan(scale), torch.ones_like(scale), scale)
    return scale


def update_oracle(w, g, v, pieces, hp, rate_num, acc, WD, track=None):
    """One step of every piece from the given sums. hp[k] = (wd, momentum) and rate_num[k] = -currentRate * trust of
    piece k. Returns (w, v, mag): fp64 tensors over the whole buffer (elements outside the pieces unchanged) and the
    magnitudes at which the ulp of each output is taken (the largest term of the sums that can cancel; "step" is
    |rate (g + wd w)|, what an error of the rate is multiplied by)."""
    w, g, v = w.to(F64).clone(), g.to(F64), v.to(F64).clone()
    scale = scale_oracle(acc, WD)
    mag = {"w": w.abs().clone(), "v": v.abs().clone(), "step": torch.zeros_like(w)}
    t = [acc.to(F64), scale]
    for k, (lo, hi, layer) in enumerate(pieces):
        wd, mom = hp[k]
        rate = rate_num[k] / float(scale[layer])
        wk, gk, vk = w[lo:hi], g[lo:hi], v[lo:hi]
        d = gk + wd * wk
        vn = mom * vk + d * rate
        mag["v"][lo:hi] = mag_of(mom * vk, rate * gk, rate * wd * wk)
        mag["w"][lo:hi] = mag_of(wk, mag["v"][lo:hi])
        mag["step"][lo:hi] = (d * rate).abs()
        t += [torch.tensor([rate], dtype=F64), wd * wk, d, mom * vk, d * rate, vn, wk - vn]
        w[lo:hi] = wk - vn
        v[lo:hi] = vn
    if track is not None:
        track.extend(t)
    return w, v, mag


def norm_chain(nchunks):
    """Roundings on the longest chain from an element to acc: a lane's running sum over its head element, 16 body
    elements and tail element (+ one for each square), the 6 shuffle steps, the 3 adds over the block's waves, then in
    the finish kernel a lane's ceil(nchunks / 64) partials and 6 more shuffle steps."""
    return 18 + 1 + 6 + 3 + (nchunks + 63) // 64 + 6


def norm_bound(total, nchunks):
    return U24 * norm_chain(nchunks) * total


def chunks_of(pieces, layer):
    return sum((hi - lo + C - 1) // C for lo, hi, ly in pieces if ly == layer)


# ------------------------------------------------------------------------------------------------ exact data
def square_vec(n, seed):
    """n integers in {0, +-1, +-2} in random order whose sum of squares is the smallest power of 4 >= n; and that
    power. From all ones (sum n) the deficit goes into twos (+3 each) after at most two zeros (-1 each)."""
    T = 1
    while T < n:
        T *= 4
    D = T - n
    zeros = (-D) % 3
    twos = (D + zeros) // 3
    assert zeros + twos <= n, (n, T)
    v = torch.ones(n, dtype=F64)
    v[:zeros] = 0.0
    v[zeros:zeros + twos] = 2.0
    g = gen(seed)
    v = v[torch.randperm(n, generator=g)]
    v = v * (torch.randint(0, 2, (n,), generator=g).to(F64) * 2 - 1)
    assert float((v ** 2).sum()) == T
    return v, T


# (WD, the steps' gradient factors): |beta| + WD is a power of two, so the scale of every step is
EXACT_WD = ((0.0, (1.0, -2.0)), (1.0, (1.0, -3.0)), (3.0, (-1.0, 1.0)))
# per-layer (wd, momentum), cycled over the layers; and rate_num = lr * trust = 0.5 * 0.5
EXACT_HP = ((0.5, 0.5), (0.0, 0.5), (0.25, 0.0), (0.0, 0.0))
EXACT_RATE = 0.25


def exact_run(lengths, WD, betas, seed, base=0):
    """Three exact steps. Steps 1 and 2 take g = beta w (so ng = |beta| nw and w, v stay multiples c w0 of the start
    pattern, whose norm is a power of two times c); the last step takes an independent integer pattern of the same
    norm as w (scaled by the layer's c), so the element-wise outputs are checked on unrelated w and g. Returns the
    pieces, the buffer length, w0, hp, [(g, acc, w_after, v_after)] in fp64 and whether every intermediate (sums,
    scale, rate, products, results) is an fp32 number."""
    pieces, n = layout(lengths, base)
    hp = [EXACT_HP[k % len(EXACT_HP)] for k in range(len(pieces))]
    rate_num = [EXACT_RATE] * len(pieces)
    w = torch.zeros(n, dtype=F64)
    pats = []
    for k, (lo, hi, _) in enumerate(pieces):
        p, _ = square_vec(hi - lo, seed + k)
        pats.append(p)
        w[lo:hi] = p
    w0, v = w.clone(), torch.zeros(n, dtype=F64)
    steps, track = [], []
    for s in range(3):
        g = torch.zeros(n, dtype=F64)
        for k, (lo, hi, _) in enumerate(pieces):
            if s < 2:
                g[lo:hi] = betas[s] * w[lo:hi]
            else:
                i = int(torch.nonzero(pats[k])[0])
                c = float(w[lo + i] / pats[k][i])
                g[lo:hi] = c * square_vec(hi - lo, seed + 1000 + k)[0]
        acc = sums_oracle(w, g, pieces, len(pieces))
        w, v, _ = update_oracle(w, g, v, pieces, hp, rate_num, acc, WD, track)
        steps.append((g, acc, w.clone(), v.clone()))
    return pieces, n, w0, hp, rate_num, steps, all(is_f32(t) for t in track)


# ------------------------------------------------------------------------------------------------ Gaussian data
GAUSS_HP = ((1e-4, 0.9), (0.0, 0.9), (5e-4, 0.0), (0.0, 0.0))
GAUSS_WD = 1e-4


def gauss_case(lengths, seed, base=0):
    """Weights ~ 0.1 N(0, 1), gradients ~ 0.01 N(0, 1), momentum ~ 1e-3 N(0, 1) as fp32; per-layer hyper-parameters
    cycled from GAUSS_HP and rates lr * trust that differ from piece to piece."""
    pieces, n = layout(lengths, base)
    q = gen(seed)
    w = (0.1 * torch.randn(n, generator=q)).to(F32)
    g = (0.01 * torch.randn(n, generator=q)).to(F32)
    v = (1e-3 * torch.randn(n, generator=q)).to(F32)
    hp = [GAUSS_HP[k % len(GAUSS_HP)] for k in range(len(pieces))]
    rate_num = [0.1 * 0.001 * (1 + k % 3) for k in range(len(pieces))]
    return pieces, n, w, g, v, hp, rate_num


def f32(x):
    """The fp32 value of a Python float (what a kernel argument or table entry holds)."""
    return float(torch.tensor(x, dtype=F32))


# ------------------------------------------------------------------------------------------------ guard cases
def guard_cases(n=C + 7, seed=11):
    """name -> (w, g, WD, expected scale): one layer each, seen through the update's outputs."""
    q = gen(seed)
    w = (0.1 * torch.randn(n, generator=q)).to(F32)
    g = (0.01 * torch.randn(n, generator=q)).to(F32)
    z = torch.zeros(n, dtype=F32)
    gn = g.clone()
    gn[n // 2] = float("nan")
    return {
        "zero_w": (z, g, GAUSS_WD, 1e4),                    # (ng + 0) / 0 = inf -> 1e4
        "zero_w_zero_g": (z, z, GAUSS_WD, 1.0),             # 0 / 0 = nan -> 1; the update is zero either way
        "tiny_g": (w * 100, g * 1e-7, 0.0, 1e-4),           # ng / nw ~ 1e-10 -> 1e-4
        "nan_g": (w, gn, GAUSS_WD, 1.0),                    # nan -> 1: the outputs carry NaN where g does
    }

