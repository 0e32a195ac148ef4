"""A/B of BinaryTreeLSTM on the fused level kernels (csrc/treelstm.hip) against the per-level torch loop: synchronised
forward + backward, host work included (the schedule and the launches are what the layer is bound by), on seeded
random binary parse trees at the sentiment example's scale: batch 128, 10-40 leaves per tree, embedding 300, hidden
150, and a second case with hidden 512. The two routes alternate inside one process; a round is the median of
``--iters`` iterations, the result the median over the rounds and the round-to-round spread (max - min).

    python tools/bench_treelstm.py [--rounds R] [--iters N] [--out FILE]
    python tools/bench_treelstm.py --once fused|loop [--hidden H]      # one iteration, for a kernel trace

The project's rule for a default: fused may become the GPU engine's default only if on both cases the gain exceeds
three times the larger of the two routes' spreads."""
import argparse
import os
import random
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_tree(k, rng, n_rows):
    """A random binary parse over k words: adjacent spans are merged in random order. Rows [left, right, tag]."""
    rows = [[0, 0, w + 1] for w in range(k)]
    spans = list(range(1, k + 1))
    while len(spans) > 1:
        i = rng.randrange(len(spans) - 1)
        rows.append([spans[i], spans[i + 1], 0])
        spans[i:i + 2] = [len(rows)]
    rows[-1][2] = -1
    return rows + [[-1, -1, -1]] * (n_rows - len(rows))


def batch(B, lo, hi, emb, seed):
    rng = random.Random(seed)
    trees = torch.tensor([parse_tree(rng.randint(lo, hi), rng, 2 * hi - 1) for _ in range(B)], dtype=torch.float32)
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, hi, emb, generator=g).cuda(), trees.cuda()


def step(m, inp, gy):
    m.forward(inp)
    m.backward(inp, gy)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", choices=["fused", "loop"], default=None)
    ap.add_argument("--hidden", type=int, default=150)
    args = ap.parse_args()
    from bigdl_amd import nn
    from bigdl_amd.ops import tree_lstm
    from bigdl_amd.utils.random_generator import RNG
    from bigdl_amd.utils.table import Table

    B, lo, hi, emb = 128, 10, 40, 300
    x, trees = batch(B, lo, hi, emb, 0)
    inp = Table(x, trees)
    lines = [f"BinaryTreeLSTM forward + backward, batch {B}, {lo}-{hi} leaves, embedding {emb}; ms per iteration "
             f"(synchronised, host included), {args.rounds} rounds of {args.iters} iterations, routes alternating"]
    for H in ([args.hidden] if args.once else [150, 512]):
        RNG.setSeed(0)
        m = nn.BinaryTreeLSTM(emb, H).cuda()
        m.training()
        gy = torch.randn(B, trees.shape[1], H, device="cuda")
        if args.once:
            tree_lstm.set_fused(args.once == "fused")
            step(m, inp, gy)
            print(f"hidden {H}: one iteration on the {tree_lstm.last_route()} route")
            return
        res = {True: [], False: []}
        for fused in (True, False):
            tree_lstm.set_fused(fused)
            step(m, inp, gy)                                 # warm-up
        for _ in range(args.rounds):
            for fused in (True, False):
                tree_lstm.set_fused(fused)
                ts = []
                for _ in range(args.iters):
                    t0 = time.perf_counter()
                    step(m, inp, gy)
                    ts.append((time.perf_counter() - t0) * 1e3)
                assert tree_lstm.last_route() == ("fused" if fused else "loop")
                res[fused].append(statistics.median(ts))
        med = {f: statistics.median(r) for f, r in res.items()}
        spread = {f: max(r) - min(r) for f, r in res.items()}
        gain, bar = med[False] - med[True], 3 * max(spread.values())
        for f in (False, True):
            lines.append(f"hidden {H:4d} {'fused' if f else 'loop '}  median {med[f]:9.3f}  spread {spread[f]:7.3f}  rounds "
                         + " ".join(f"{t:.3f}" for t in res[f]))
        lines.append(f"hidden {H:4d} gain {gain:9.3f} ms ({med[False] / med[True]:.2f}x), 3 x larger spread {bar:.3f}: "
                     f"{'passes' if gain > bar else 'does not pass'} the rule for a default")
    tree_lstm.set_fused(None)
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
