#!/usr/bin/env python
"""A/B of the sparse modules with the native kernels off / on (BIGDL_SPARSE_NATIVE 0 / 1: torch.sparse.mm and
to_dense / to_sparse against csrc/sparse.hip), each case one synchronised forward plus backward on cuda:0.

  python tools/bench_sparse.py                 all cases, report written to profiles/sparse_native_ab.txt
  python tools/bench_sparse.py --cases lookup --out FILE

Cases:
  wide        SparseJoinTable(2) -> SparseLinear(10^6, 2), batch 8192, two inputs of 5 * 10^5 columns with 20 entries
              per row each: the wide half of a Wide & Deep model at its real size
  wide_small  the same with two inputs of 2000 columns, small enough for the dense temporaries of the torch route
  lookup      LookupTableSparse(10^5, 64), batch 8192, 10 ids per row

Each round times ``--iters`` iterations of one route, then of the other; the report gives the median over ``--rounds``
rounds and the round-to-round spread (max - min). A route whose warm-up iteration takes longer than ``--slow``
seconds is timed with fewer iterations per round (said in the report); a route that runs out of memory is reported
as such and counts as a gain for the other. Native is worth its default for a module only when it wins by more than
three times the larger spread; the verdict says so.
"""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

CASES = ["wide", "wide_small", "lookup"]


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--cases", default=",".join(CASES))
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--slow", type=float, default=0.5, help="seconds per iteration above which a route gets fewer iterations")
    p.add_argument("--out", default=os.path.join(HERE, "profiles", "sparse_native_ab.txt"))
    return p.parse_args()


def random_rows(B, D, per_row, g):
    """A coalesced [B, D] sparse tensor with (up to) ``per_row`` entries per row and values in (0.5, 1.5)."""
    import torch

    rows = torch.arange(B).repeat_interleave(per_row)
    cols = torch.randint(0, D, (B * per_row,), generator=g)
    vals = torch.rand(B * per_row, generator=g) + 0.5
    return torch.sparse_coo_tensor(torch.stack([rows, cols]), vals, (B, D)).coalesce()


def make(case):
    """(step, note): step() is one forward plus backward; note describes the workload."""
    import torch

    from bigdl_amd import nn
    from bigdl_amd.utils.table import T

    g = torch.Generator().manual_seed(1)
    dev = torch.device("cuda")
    B = 8192
    if case in ("wide", "wide_small"):
        D = 500000 if case == "wide" else 2000
        xs = [random_rows(B, D, 20, g) for _ in range(2)]
        nnz = [x._nnz() for x in xs]
        inp = T(*[x.to(dev) for x in xs])
        model = nn.Sequential().add(nn.SparseJoinTable(2)).add(nn.SparseLinear(2 * D, 2)).to(dev)
        gy = torch.randn(B, 2, generator=g).to(dev)
        note = (f"SparseJoinTable(2) -> SparseLinear({2 * D}, 2), batch {B}, two inputs of {D} columns, nnz {nnz}; "
                f"dense join would be {B * 2 * D * 4 / 2 ** 30:.1f} GiB")
    elif case == "lookup":
        where = torch.stack([torch.arange(B).repeat_interleave(10), torch.arange(10).repeat(B)])
        ids = torch.sparse_coo_tensor(where, torch.randint(1, 100001, (B * 10,), generator=g).float(),
                                      (B, 10)).coalesce()
        inp = ids.to(dev)
        model = nn.LookupTableSparse(100000, 64, "sum").to(dev)
        gy = torch.randn(B, 64, generator=g).to(dev)
        note = f"LookupTableSparse(100000, 64, sum), batch {B}, nnz {ids._nnz()}"
    else:
        raise ValueError(f"unknown case {case!r}; known: {CASES}")

    def step():
        model.forward(inp)
        model.backward(inp, gy)
        torch.cuda.synchronize()

    return step, note


def timed(step, native, iters):
    """Seconds per iteration of ``iters`` iterations on one route, or None when the route runs out of memory."""
    import torch

    from bigdl_amd.ops import sparse as sp

    sp.set_native(bool(native))
    try:
        t0 = time.perf_counter()
        for _ in range(iters):
            step()
        return (time.perf_counter() - t0) / iters
    except torch.cuda.OutOfMemoryError:
        torch.cuda.empty_cache()
        return None
    finally:
        sp.set_native(None)


def main():
    a = parse()
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    say(f"bench_sparse: ms per synchronised forward + backward, {a.rounds} rounds of {a.iters} iterations per route, "
        f"alternating torch / native in one process; median of the rounds, spread = max - min of the rounds")
    for case in a.cases.split(","):
        step, note = make(case)
        say(f"{case}: {note}")
        iters, oom = {}, {}
        for route in (0, 1):                                 # warm-up: kernel load, caches, allocator
            w = timed(step, route, 1)
            oom[route] = w is None
            if not oom[route]:
                w = timed(step, route, 1)
            iters[route] = a.iters if (w is None or w <= a.slow) else max(1, min(a.iters, int(a.slow * a.iters / w)))
        times = {0: [], 1: []}
        for _ in range(a.rounds):
            for route in (0, 1):
                if not oom[route]:
                    t = timed(step, route, iters[route])
                    if t is None:
                        oom[route] = True
                    else:
                        times[route].append(t * 1e3)
        med, spread = {}, {}
        for route, name in ((0, "torch "), (1, "native")):
            if oom[route] or not times[route]:
                say(f"  {name} out of memory: the route cannot run this case")
                continue
            med[route] = statistics.median(times[route])
            spread[route] = max(times[route]) - min(times[route])
            say(f"  {name} {med[route]:10.3f} ms  spread {spread[route]:8.3f} ms  rounds "
                + " ".join(f"{t:.3f}" for t in times[route])
                + (f"  ({iters[route]} iterations per round: slow route)" if iters[route] != a.iters else ""))
        if 0 in med and 1 in med:
            wins = med[0] - med[1] > 3 * max(spread.values())
            say(f"  torch / native {med[0] / med[1]:.2f}x; gain {med[0] - med[1]:.3f} ms against 3 x spread "
                f"{3 * max(spread.values()):.3f} ms: native {'wins' if wins else 'does not win'}")
        elif 1 in med:
            say("  only the native route runs this case: native wins")
        else:
            say("  the native route did not run this case")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
