"""A/B timing of Recurrent(ConvLSTMPeephole) on the GPU: the fused step kernels (csrc/convlstm.hip, _ConvLSTMSeq)
against the Python time loop (BIGDL_CONVLSTM_FUSED=0), both in this process and this build, alternating windows.

    python tools/bench_convlstm.py [--out FILE]

Times one training step (forward + backward with parameter gradients) of the module per shape with device events
around windows of --iters steps; prints the median and the range over --windows windows per side, and the relative L2
difference of the two sides' output and input gradient on the same seeded input."""
import argparse
import copy
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bigdl_amd import nn  # noqa: E402
from bigdl_amd.nn import recurrent  # noqa: E402

# B, T, Cin, C, H, W, kernel
SHAPES = [(8, 10, 16, 64, 64, 64, 3), (8, 10, 16, 64, 64, 64, 5), (16, 10, 1, 32, 32, 32, 3),
          (4, 5, 16, 256, 32, 32, 3)]      # four channel tiles: every one re-stages the 4C-channel halo in backward


def step(m, x, gy):
    y = m.forward(x)
    return y, m.backward(x, gy)


def window(m, x, gy, iters):
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    for _ in range(iters):
        step(m, x, gy)
    end.record()
    end.synchronize()
    return beg.elapsed_time(end) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [f"ConvLSTMPeephole A/B, forward + backward of Recurrent(ConvLSTMPeephole): device events, {a.windows} "
             f"alternating windows of {a.iters} steps, ms per step: median [min .. max]"]
    for B, T, Cin, C, H, W, k in SHAPES:
        torch.manual_seed(0)
        m = nn.Recurrent().add(nn.ConvLSTMPeephole(Cin, C, k, k)).to("cuda")
        side = {True: m, False: copy.deepcopy(m)}
        x = torch.randn(B, T, Cin, H, W, device="cuda").bfloat16().float()
        gy = torch.randn(B, T, C, H, W, device="cuda")
        times, res = {True: [], False: []}, {}
        for fused in (True, False):                          # warm-up of both sides, and their results
            recurrent._CONVLSTM_FUSED[0] = fused
            res[fused] = [t.clone() for t in step(side[fused], x, gy)]
            window(side[fused], x, gy, 2)
        for _ in range(a.windows):
            for fused in (True, False):
                recurrent._CONVLSTM_FUSED[0] = fused
                times[fused].append(window(side[fused], x, gy, a.iters))
        recurrent._CONVLSTM_FUSED[0] = True
        # the recurrent convolution only: 2 (fwd) + 4 (dgrad, wgrad) x B T H W 4C C k^2
        flops = 6.0 * B * T * H * W * 4 * C * C * k * k
        lines.append(f"B={B} T={T} Cin={Cin} C={C} {H}x{W} kernel {k}x{k}")
        for fused in (True, False):
            t = times[fused]
            med = statistics.median(t)
            lines.append(f"  {'fused' if fused else 'loop '} {med:9.3f} [{min(t):9.3f} .. {max(t):9.3f}]  "
                         f"{flops / med / 1e9:6.1f} TFLOP/s of recurrent convolution, end to end")
        lines.append(f"  loop / fused = {statistics.median(times[False]) / statistics.median(times[True]):.2f}")
        for name, p, q in zip(("output", "input gradient"), res[True], res[False]):
            lines.append(f"  |fused - loop| / |loop| of {name}: {((p - q).norm() / q.norm()).item():.3e}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
