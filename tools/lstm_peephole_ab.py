"""A/B of the fused LSTMPeephole / maskZero LSTM sequence path (csrc/lstm.hip) against the Python time loop
(Cell.sequence): forward + backward of Recurrent(LSTMPeephole(1024, 1024)) and Recurrent(maskZero=True)(LSTM(1024,
1024)) at B = 128, T = 64 in training mode, input lengths of the masked case spread over [T/2, T].

    python tools/lstm_peephole_ab.py [--tree DIR] [--iters N] [--reps R]

--tree DIR imports bigdl_amd from another checkout (e.g. the parent commit, which only has the loop)."""
import argparse
import os
import statistics
import sys

import torch


def time_module(m, x, iters, reps):
    gy = torch.randn(x.shape[0], x.shape[1], 1024, device=x.device)
    for _ in range(3):
        m.forward(x)
        m.backward(x, gy)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            m.forward(x)
            m.backward(x, gy)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / iters)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    sys.path.insert(0, args.tree)
    from bigdl_amd import nn
    from bigdl_amd.nn import recurrent as rc
    from bigdl_amd.utils.random_generator import RNG

    switch = getattr(rc, "_PEEP_FUSED", None)
    B, T, I, H = 128, 64, 1024, 1024
    RNG.setSeed(0)
    torch.manual_seed(0)
    x = torch.randn(B, T, I, device="cuda")
    xm = x.clone()
    for b in range(B):
        xm[b, T // 2 + (b * 5) % (T // 2 + 1):] = 0
    cases = [("Recurrent(LSTMPeephole(1024, 1024))", nn.Recurrent().add(nn.LSTMPeephole(I, H)).cuda(), x),
             ("Recurrent(maskZero)(LSTM(1024, 1024))", nn.Recurrent(maskZero=True).add(nn.LSTM(I, H)).cuda(), xm)]
    print(f"tree={args.tree} fused path present: {switch is not None}; B={B} T={T}; ms per forward+backward, "
          f"{args.reps} windows of {args.iters} iterations")
    for name, m, inp in cases:
        m.training()
        res = {}
        for rnd in range(2):                       # alternate the two paths: drift shows as a gap between rounds
            for fused in ([True, False] if switch is not None else [False]):
                if switch is not None:
                    switch[0] = fused
                res.setdefault(fused, []).extend(time_module(m, inp, args.iters, args.reps))
        if switch is not None:
            switch[0] = True
        for fused, ts in res.items():
            print(f"{name:40s} {'fused ' if fused else 'loop  '} median {statistics.median(ts):8.3f}  "
                  f"min {min(ts):8.3f}  max {max(ts):8.3f}")


if __name__ == "__main__":
    main()
