"""A/B timing of Recurrent(ConvLSTMPeephole) on the GPU: the fused step kernels (csrc/convlstm.hip, _ConvLSTMSeq)
against the Python time loop (BIGDL_CONVLSTM_FUSED=0), both in this process and this build, alternating windows.
``--nd 3``: Recurrent(ConvLSTMPeephole3D), the opt-in fused route (csrc/convlstm3d.hip, _ConvLSTM3dSeq) against the loop.

    python tools/bench_convlstm.py [--nd 2|3] [--out FILE]

Times one training step (forward + backward with parameter gradients) of the module per shape with device events
around windows of --iters steps; prints the median and the range over --windows windows per side, and the relative L2
difference of the two sides' output and input gradient on the same seeded input."""
import argparse
import copy
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bigdl_amd import nn  # noqa: E402
from bigdl_amd.nn import recurrent  # noqa: E402

# B, T, Cin, C, H, W, kernel
SHAPES = {2: [(8, 10, 16, 64, 64, 64, 3), (8, 10, 16, 64, 64, 64, 5), (16, 10, 1, 32, 32, 32, 3),
              (4, 5, 16, 256, 32, 32, 3)],     # four channel tiles: every one re-stages the 4C-channel halo in backward
          # B, T, Cin, C, D, H, W, kernel: video volumes
          3: [(4, 8, 16, 64, 16, 32, 32, 3), (2, 8, 16, 128, 8, 32, 32, 3), (4, 8, 16, 64, 8, 16, 16, 3),
              (2, 4, 8, 32, 8, 24, 24, 5)]}
CELL = {2: nn.ConvLSTMPeephole, 3: nn.ConvLSTMPeephole3D}


def set_fused(nd, on):
    if nd == 2:
        recurrent._CONVLSTM_FUSED[0] = on
    else:
        recurrent.set_convlstm3d_fused(on)


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
    ap.add_argument("--nd", type=int, default=2, choices=(2, 3))
    a = ap.parse_args()
    cell = CELL[a.nd].__name__
    lines = [f"{cell} A/B, forward + backward of Recurrent({cell}): device events, {a.windows} "
             f"alternating windows of {a.iters} steps, ms per step: median [min .. max]"]
    for B, T, Cin, C, *vol, k in SHAPES[a.nd]:
        torch.manual_seed(0)
        m = nn.Recurrent().add(CELL[a.nd](Cin, C, k, k)).to("cuda")
        side = {True: m, False: copy.deepcopy(m)}
        x = torch.randn(B, T, Cin, *vol, device="cuda").bfloat16().float()
        gy = torch.randn(B, T, C, *vol, device="cuda")
        times, res = {True: [], False: []}, {}
        for fused in (True, False):                          # warm-up of both sides, and their results
            set_fused(a.nd, fused)
            res[fused] = [t.clone() for t in step(side[fused], x, gy)]
            window(side[fused], x, gy, 2)
        for _ in range(a.windows):
            for fused in (True, False):
                set_fused(a.nd, fused)
                times[fused].append(window(side[fused], x, gy, a.iters))
        set_fused(a.nd, True if a.nd == 2 else None)
        # the recurrent convolution only: 2 (fwd) + 4 (dgrad, wgrad) x B T (D) H W 4C C k^nd
        flops = 6.0 * B * T * math.prod(vol) * 4 * C * C * k ** a.nd
        lines.append(f"B={B} T={T} Cin={Cin} C={C} {'x'.join(map(str, vol))} kernel {'x'.join([str(k)] * a.nd)}")
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
