"""A/B timing of grouped nn.SpatialConvolution on the GPU: every group in one MFMA launch per pass
(csrc/gconv_mfma.hip, conv_fn.set_gconv_mfma(True)) against the default routes (the direct kernel up to 16 input
channels per group, else one implicit-GEMM convolution per group), both in this process and this build, alternating
windows.

    python tools/bench_gconv.py [--out FILE]

Times forward, data gradient (updateGradInput) and weight gradient (accGradParameters) of the 3 x 3 layers of
ResNeXt-50 32x4d / 32x8d with 8 .. 64 channels per group at their feature-map sizes and of the two-group AlexNet
layers, batch 32, bf16 NHWC activations as inside a model, with device events around windows of calls sized to about
--window seconds; prints the median and the range over --rounds rounds per side, the gain, the larger round-to-round
spread, and the largest difference between the two sides' results on the same inputs."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bigdl_amd import nn  # noqa: E402
from bigdl_amd.ops import conv_fn  # noqa: E402

# name, N, Cin, Cout, groups, H = W, kernel, pad
SHAPES = [("resnext 32x4d cin_g=8", 32, 256, 256, 32, 28, 3, 1), ("resnext 32x4d cin_g=16", 32, 512, 512, 32, 14, 3, 1),
          ("resnext 32x4d cin_g=32", 32, 1024, 1024, 32, 7, 3, 1),
          ("resnext 32x8d cin_g=8", 32, 256, 256, 32, 56, 3, 1), ("resnext 32x8d cin_g=16", 32, 512, 512, 32, 28, 3, 1),
          ("resnext 32x8d cin_g=32", 32, 1024, 1024, 32, 14, 3, 1),
          ("resnext 32x8d cin_g=64", 32, 2048, 2048, 32, 7, 3, 1), ("alexnet conv2", 32, 96, 256, 2, 27, 5, 2),
          ("alexnet conv4", 32, 384, 384, 2, 13, 3, 1), ("alexnet conv5", 32, 384, 256, 2, 13, 3, 1)]


def run(m, x, gy, what):
    if what == "fwd  ":
        return m.forward(x)
    if what == "dgrad":
        return m.updateGradInput(x, gy)
    m.gradWeight.zero_()
    m.accGradParameters(x, gy)
    return m.gradWeight


def window(args, iters):
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    for _ in range(iters):
        run(*args)
    end.record()
    end.synchronize()
    return beg.elapsed_time(end) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.2, help="seconds of calls per timing window")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [f"grouped conv A/B: mfma (csrc/gconv_mfma.hip, one launch per pass) vs base (direct kernel / per-group "
             f"loop); device events, {a.rounds} alternating rounds of ~{a.window} s windows (2000 calls at most), ms "
             f"per call: median [min .. max]; gain = base / mfma - 1, spread = the larger (max - min) / median of the "
             f"two sides"]
    for name, N, Cin, Cout, G, HW, k, p in SHAPES:
        torch.manual_seed(0)
        m = nn.SpatialConvolution(Cin, Cout, k, k, 1, 1, p, p, nGroup=G).to("cuda")
        x = torch.randn(N, Cin, HW, HW, device="cuda").to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        gy = None
        for what in ("fwd  ", "dgrad", "wgrad"):
            out, times, iters, route = {}, {True: [], False: []}, {}, {}
            for on in (True, False):                      # warm-up of both sides, their results, and the window size
                conv_fn.set_gconv_mfma(on)
                m.forward(x)                              # the backward passes read what this side's forward kept
                if gy is None:
                    gy = torch.randn_like(m.output)
                args = (m, x, gy, what)
                out[on] = run(*args).float().clone()
                route[on] = conv_fn.last_group_route()
                iters[on] = max(3, min(2000, int(a.window * 1e3 / max(window(args, 3), 1e-3))))
            if route[True] != "mfma":
                lines.append(f"{name} {what} mfma route not taken: base only")
                continue
            for _ in range(a.rounds):
                for on in (True, False):
                    conv_fn.set_gconv_mfma(on)
                    m.forward(x)
                    times[on].append(window((m, x, gy, what), iters[on]))
            med = {f: statistics.median(times[f]) for f in (True, False)}
            spread = max((max(times[f]) - min(times[f])) / med[f] for f in (True, False))
            diff = ((out[True] - out[False]).abs().max() / out[False].abs().max()).item()
            lines.append(f"{name} N={N} {Cin}->{Cout} G={G} {HW}x{HW} k={k} {what} mfma {med[True]:8.3f} "
                         f"[{min(times[True]):8.3f} .. {max(times[True]):8.3f}]  base({route[False]}) "
                         f"{med[False]:8.3f} [{min(times[False]):8.3f} .. {max(times[False]):8.3f}]  "
                         f"gain {med[False] / med[True] - 1:+7.1%}  spread {spread:6.1%}  max rel diff {diff:.2e}")
            print(lines[-1], flush=True)
    conv_fn.set_gconv_mfma(None)
    text = "\n".join(lines)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
