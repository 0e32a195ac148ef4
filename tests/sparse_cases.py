"""Cases, data and fp64 oracles for the sparse kernels (csrc/sparse.hip, bigdl_amd/ops/sparse.py), shared by
tests/test_sparse_gpu.py (kernel vs oracle, element by element) and tests/test_sparse_cpu.py (the oracles' own sanity,
the torch forms, and that every case holds the edge it names). Everything here runs on the CPU.

A pattern is a coalesced COO list: int64 rows / cols in row-major order. The oracles are plain loops over that list
in fp64 (vectorised over the output axis only), and like the kernels they skip an entry whose row is outside [0, B),
whose column is outside [0, D) or whose id is outside [1, nIndex].

Two legs:

* exact: small integers (values and ids' weights in [-3, 3] without 0, W and gy in [-4, 4], bias in [-8, 8]). Every
  product and partial sum is an integer far below 2^24 (the longest sum has 130 terms of at most 12, the widest
  contended column 67 rows), so fp32 is exact whatever the order: atomics or ordered, results are defined bit for bit.
* gauss: Gaussian data against fp64. A fixed-order or atomic fp32 sum of n products with one final scale:
  per element |err| <= (n + 4) * 2^-23 * sum |terms| (``bound``), n = that element's number of contributions and the
  sum of absolute terms computed in fp64, scale included. For the mean / sqrtn combiners the weights are positive, so
  the row scale's own n-term sum has no cancellation and stays inside the same bound.
"""
import functools
from dataclasses import dataclass

import torch

U23 = 2.0 ** -23
BIG_D = 100003
N_SIZES = (1, 2, 3, 64, 65)
NOUT_SIZES = (1, 63, 64, 130)
HOT = 7                      # the column every row of the "contended" case hits


def bound(n, abs_terms):
    """(n + 4) * 2^-23 * sum |terms|, fp64; n and abs_terms broadcast."""
    return (n.double() + 4.0) * U23 * abs_terms.double()


@dataclass(frozen=True)
class Case:
    name: str
    B: int
    D: int
    counts: tuple              # entries per row
    hot: int = -1              # a column present in every non-empty row, or -1

    @property
    def nnz(self):
        return sum(self.counts)


def _filler(B, special, seed, lo=0):
    g = torch.Generator().manual_seed(seed)
    c = torch.randint(lo, 21, (B,), generator=g).tolist()
    for i, v in special.items():
        c[i % B] = v
    return tuple(c)


CASES = (
    Case("b1_130", 1, BIG_D, (130,)),
    Case("b5_edges", 5, BIG_D, (0, 63, 64, 65, 0)),
    Case("b5_one_row", 5, BIG_D, (0, 0, 130, 0, 0)),
    Case("b5_empty", 5, BIG_D, (0, 0, 0, 0, 0)),
    Case("b67_mixed", 67, BIG_D, _filler(67, {0: 0, 1: 1, 2: 63, 3: 64, 4: 65, 5: 130, 66: 0}, 1)),
    Case("b67_contended", 67, BIG_D, _filler(67, {0: 1, 3: 64, 66: 5}, 2, lo=1), hot=HOT),
    Case("b67_d1", 67, 1, tuple(0 if b in (0, 66) else 1 for b in range(67)), hot=0),
)
CASE = {c.name: c for c in CASES}


@functools.lru_cache(maxsize=None)
def pattern(name):
    """(rows, cols) int64 of the case: per row ``counts[b]`` distinct ascending columns; a row with at least two
    entries holds columns 0 and D - 1, every non-empty row holds ``hot``."""
    c = CASE[name]
    g = torch.Generator().manual_seed(1000 + CASES.index(c))
    rows, cols = [], []
    for b, k in enumerate(c.counts):
        if k == 0:
            continue
        if k > c.D:
            raise ValueError("more entries than columns")
        must = set()
        if c.hot >= 0:
            must.add(c.hot)
        if k >= 2 + len(must) and c.D >= 2:
            must |= {0, c.D - 1}
        pick = set(must)
        while len(pick) < k:
            pick.add(int(torch.randint(0, c.D, (1,), generator=g)))
        cols += sorted(pick)
        rows += [b] * k
    return torch.tensor(rows, dtype=torch.int64), torch.tensor(cols, dtype=torch.int64)


def ints(shape, lo, hi, seed, nonzero=False):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(lo, hi + 1, tuple(shape), generator=g).float()
    if nonzero:
        t = torch.where(t == 0, torch.ones_like(t), t)
    return t


def gauss(shape, seed, positive=False):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(tuple(shape), generator=g)
    return t.abs() + 0.25 if positive else t


def sparse(rows, cols, vals, B, D, device="cpu", coalesced=True):
    """The torch tensor of a COO list, built without index validation (an out-of-range index stays as it is)."""
    idx = torch.stack([rows, cols]).to(device)
    return torch.sparse_coo_tensor(idx, vals.to(device), (B, D), check_invariants=False, is_coalesced=coalesced)


def dense(rows, cols, vals, B, D):
    out = torch.zeros(B, D, dtype=torch.float64)
    for r, c, v in zip(rows.tolist(), cols.tolist(), vals.tolist()):
        if 0 <= r < B and 0 <= c < D:
            out[r, c] += v
    return out


# --------------------------------------------------------------------------------------------- oracles (fp64 loops)
def spmm_oracle(rows, cols, vals, W, bias, B):
    """(y, sum |terms|, n) of y[b, o] = bias[o] + sum_k val_k W[o, col_k]; n counts the bias as one contribution."""
    N, D = W.shape
    W = W.double()
    y = torch.zeros(B, N, dtype=torch.float64)
    a = torch.zeros(B, N, dtype=torch.float64)
    n = torch.zeros(B, 1, dtype=torch.float64)
    if bias is not None:
        y += bias.double()
        a += bias.double().abs()
        n += 1
    for r, c, v in zip(rows.tolist(), cols.tolist(), vals.tolist()):
        if not (0 <= r < B and 0 <= c < D):
            continue
        t = v * W[:, c]
        y[r] += t
        a[r] += t.abs()
        n[r] += 1
    return y, a, n


def wgrad_oracle(rows, cols, vals, gy, D, scale=1.0):
    """(g, sum |terms|, n) of g[o, col_k] += scale val_k gy[row_k, o] from zero; n [1, D]."""
    B, N = gy.shape
    gy = gy.double()
    g = torch.zeros(N, D, dtype=torch.float64)
    a = torch.zeros(N, D, dtype=torch.float64)
    n = torch.zeros(1, D, dtype=torch.float64)
    for r, c, v in zip(rows.tolist(), cols.tolist(), vals.tolist()):
        if not (0 <= r < B and 0 <= c < D):
            continue
        t = scale * v * gy[r]
        g[:, c] += t
        a[:, c] += t.abs()
        n[0, c] += 1
    return g, a, n


def sddmm_oracle(rows, cols, gy, W):
    """(g, sum |terms|, n) of g_k = sum_o gy[row_k, o] W[o, col_k]; a skipped entry gets 0."""
    B, N = gy.shape
    D = W.shape[1]
    gy, W = gy.double(), W.double()
    g = torch.zeros(rows.numel(), dtype=torch.float64)
    a = torch.zeros(rows.numel(), dtype=torch.float64)
    for k, (r, c) in enumerate(zip(rows.tolist(), cols.tolist())):
        if not (0 <= r < B and 0 <= c < D):
            continue
        t = gy[r] * W[:, c]
        g[k], a[k] = t.sum(), t.abs().sum()
    return g, a, torch.full((rows.numel(),), float(N), dtype=torch.float64)


def lookup_oracle(rows, ids, wts, W, combiner, B):
    """(out, scales, sum |terms|, n) of out[b] = s_b sum_k w_k W[id_k - 1]."""
    nIndex, nOut = W.shape
    W = W.double()
    acc = torch.zeros(B, nOut, dtype=torch.float64)
    a = torch.zeros(B, nOut, dtype=torch.float64)
    n = torch.zeros(B, 1, dtype=torch.float64)
    den = torch.zeros(B, dtype=torch.float64)
    w_all = torch.ones(ids.numel(), dtype=torch.float64) if wts is None else wts.double()
    for r, i, w in zip(rows.tolist(), ids.tolist(), w_all.tolist()):
        i = int(i)
        if not (0 <= r < B and 1 <= i <= nIndex):
            continue
        t = w * W[i - 1]
        acc[r] += t
        a[r] += t.abs()
        n[r] += 1
        den[r] += w if combiner == "mean" else w * w
    s = torch.ones(B, dtype=torch.float64)
    if combiner == "mean":
        s = torch.where(den != 0, 1.0 / den, torch.zeros_like(den))
    elif combiner == "sqrtn":
        s = torch.where(den > 0, den.rsqrt(), torch.zeros_like(den))
    return acc * s[:, None], s, a * s.abs()[:, None], n


def lookup_bwd_oracle(rows, ids, wts, scales, gy, nIndex, scale=1.0):
    """(g, sum |terms|, n) of g[id_k - 1] += scale s_b w_k gy[b] from zero; n [nIndex, 1]."""
    B, nOut = gy.shape
    gy, scales = gy.double(), scales.double()
    g = torch.zeros(nIndex, nOut, dtype=torch.float64)
    a = torch.zeros(nIndex, nOut, dtype=torch.float64)
    n = torch.zeros(nIndex, 1, dtype=torch.float64)
    w_all = torch.ones(ids.numel(), dtype=torch.float64) if wts is None else wts.double()
    for r, i, w in zip(rows.tolist(), ids.tolist(), w_all.tolist()):
        i = int(i)
        if not (0 <= r < B and 1 <= i <= nIndex):
            continue
        t = scale * scales[r] * w * gy[r]
        g[i - 1] += t
        a[i - 1] += t.abs()
        n[i - 1] += 1
    return g, a, n


def concat_oracle(parts, B):
    """parts = [(rows, cols, vals, D_i)]; (rows, cols, vals) of the join along the columns: row by row, input by
    input, columns shifted by the widths before."""
    per = []
    for rows, cols, vals, _ in parts:
        by = [[] for _ in range(B)]
        for r, c, v in zip(rows.tolist(), cols.tolist(), vals.tolist()):
            by[r].append((c, v))
        per.append(by)
    orows, ocols, ovals = [], [], []
    for b in range(B):
        shift = 0
        for by, (_, _, _, D) in zip(per, parts):
            for c, v in by[b]:
                orows.append(b)
                ocols.append(c + shift)
                ovals.append(v)
            shift += D
    return (torch.tensor(orows, dtype=torch.int64), torch.tensor(ocols, dtype=torch.int64),
            torch.tensor(ovals, dtype=torch.float32))


# --------------------------------------------------------------------------------------------- lookup / join cases
N_INDEX = 50


@functools.lru_cache(maxsize=None)
def lookup_pattern(name):
    """(rows, slots, ids): the case's row lengths with the columns as slot positions 0 .. count - 1 (a [B, 130]
    id tensor) and ids in [1, N_INDEX]; in a contended case every non-empty row's first id is HOT."""
    c = CASE[name]
    g = torch.Generator().manual_seed(2000 + CASES.index(c))
    rows, slots, ids = [], [], []
    for b, k in enumerate(c.counts):
        for j in range(k):
            rows.append(b)
            slots.append(j)
            ids.append(HOT if (c.hot >= 0 and j == 0) else int(torch.randint(1, N_INDEX + 1, (1,), generator=g)))
    return (torch.tensor(rows, dtype=torch.int64), torch.tensor(slots, dtype=torch.int64),
            torch.tensor(ids, dtype=torch.float32))


LOOKUP_L = 130

# joins: (name, B, [(case name or None for an empty input, width)]): 1, 2, 3 and 8 inputs, an input without entries,
# inputs of different widths
JOINS = (
    ("one", 5, (("b5_edges", BIG_D),)),
    ("two", 67, (("b67_mixed", BIG_D), ("b67_d1", 1))),
    ("three_with_empty", 5, (("b5_edges", BIG_D), ("b5_empty", BIG_D), ("b5_one_row", BIG_D))),
    ("eight", 67, (("b67_mixed", BIG_D), ("b67_d1", 1), ("b67_contended", BIG_D), ("b67_d1", 1),
                   ("b67_mixed", BIG_D), ("b67_contended", BIG_D), ("b67_d1", 1), ("b67_mixed", BIG_D))),
    ("all_empty", 5, (("b5_empty", BIG_D), ("b5_empty", BIG_D))),
)


def join_parts(name, exact=True):
    _, B, members = next(j for j in JOINS if j[0] == name)
    parts = []
    for i, (cname, D) in enumerate(members):
        rows, cols = pattern(cname)
        vals = ints((rows.numel(),), -3, 3, 300 + i, nonzero=True) if exact else gauss((rows.numel(),), 300 + i)
        parts.append((rows, cols, vals, D))
    return B, parts
