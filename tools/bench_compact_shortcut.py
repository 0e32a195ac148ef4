"""Per-stage cost of a ResNet-50 projection shortcut's gradient (batch 256, one MI355X), materialised vs compact.

For the three downsampling blocks it times (CUDA events, median of --iters launches) the two kernels the shortcut
gradient passes through in the backward step:
  * the shortcut's 1x1 / stride-2 data gradient: dgrad_fill + strided phase GEMM at the input resolution, or one
    dense GEMM at the output resolution (ops/conv.py conv2d_dgrad ``compact``);
  * the data gradient of the branch's first 1x1 convolution, which adds it in its epilogue (with the consumer-BN
    reduction under a sign mask, as in the step): a full-resolution addend, or the compact one read subsampled
    (csrc/kernels.h ConvArgs::add_sh).

    python tools/bench_compact_shortcut.py [--batch 256] [--iters 30]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bigdl_amd  # noqa: F401,E402
from bigdl_amd.ops import bn as bnops  # noqa: E402
from bigdl_amd.ops import conv as cv  # noqa: E402
from conv_roofline import timed  # noqa: E402

# (block input channels, input H, branch width, shortcut output channels)
STAGES = [(256, 56, 128, 512), (512, 28, 256, 1024), (1024, 14, 512, 2048)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=30)
    a = ap.parse_args()
    N, dev = a.batch, torch.device("cuda")
    CL, BF = torch.channels_last, torch.bfloat16
    print(f"{'C':>5} {'HxW':>7} {'n':>4} {'Ks':>5}  {'short full':>10} {'short cmp':>10} {'first full':>10} "
          f"{'first cmp':>10} {'sum full':>9} {'sum cmp':>9}   (us)")
    tot = [0.0, 0.0]
    for C, H, n, Ks in STAGES:
        OH = H // 2
        ws = cv.transpose_w((torch.randn(Ks, C, 1, 1, device=dev) * 0.05).to(BF, memory_format=CL))
        wf = cv.transpose_w((torch.randn(n, C, 1, 1, device=dev) * 0.05).to(BF, memory_format=CL))
        gs = torch.randn(N, Ks, OH, OH, device=dev).to(BF, memory_format=CL)
        gf = torch.randn(N, n, H, H, device=dev).to(BF, memory_format=CL)
        bx = torch.randn(N, C, H, H, device=dev).to(BF, memory_format=CL)
        zm = torch.randint(0, 256, (N * H * H, C // 8), device=dev, dtype=torch.uint8)
        mean, aff = torch.zeros(C, device=dev), torch.ones(2 * C, device=dev)
        shape = (N, C, H, H)
        full = cv.conv2d_dgrad(gs, ws, shape, (2, 2), (0, 0))
        comp = cv.conv2d_dgrad(gs, ws, shape, (2, 2), (0, 0), compact=True)
        assert cv.addend_stride_applies(N, n, H, H, C, (2, 2), 1), "no kernel takes the compact addend here"

        def first(addend):
            bn = {"x": bx, "z": None, "zm": zm, "mean": mean, "aff": aff, "red": bnops.new_stats(C, dev)}
            return cv.conv2d_dgrad(gf, wf, shape, (1, 1), (0, 0), addend=addend, bn=bn)

        assert torch.equal(first(full), first(comp))
        t = [timed(lambda: cv.conv2d_dgrad(gs, ws, shape, (2, 2), (0, 0)), a.iters),
             timed(lambda: cv.conv2d_dgrad(gs, ws, shape, (2, 2), (0, 0), compact=True), a.iters),
             timed(lambda: first(full), a.iters), timed(lambda: first(comp), a.iters)]
        tot[0] += t[0] + t[2]
        tot[1] += t[1] + t[3]
        print(f"{C:>5} {H:>3}x{H:<3} {n:>4} {Ks:>5}  {t[0]:>10.1f} {t[1]:>10.1f} {t[2]:>10.1f} {t[3]:>10.1f} "
              f"{t[0] + t[2]:>9.1f} {t[1] + t[3]:>9.1f}", flush=True)
    print(f"# three blocks: materialised {tot[0]:.1f} us, compact {tot[1]:.1f} us, saved {tot[0] - tot[1]:.1f} us")


if __name__ == "__main__":
    main()
