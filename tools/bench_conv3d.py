"""A/B timing of 3-D convolution on the GPU: the native kernels (csrc/conv3d.hip) against the per-temporal-tap path
(BIGDL_CONV3D_NATIVE=0), both in this process and this build, alternating windows.

    python tools/bench_conv3d.py [--out FILE]

Times forward, and forward + backward, of one video-model layer with device events around windows of --iters calls;
prints the median and the range over --windows windows per side, and the largest difference between the two sides'
results on the same seeded inputs."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bigdl_amd.ops import conv_fn  # noqa: E402


def run(x, w, b, gy, stride, pad, backward):
    y = conv_fn.conv3d(x, w, b, stride, pad)
    if not backward:
        return (y,)
    return (y,) + torch.autograd.grad(y, (x, w, b), gy)


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
    ap.add_argument("--shape", type=int, nargs=6, default=[8, 64, 128, 16, 56, 56], metavar=tuple("NCKTHW"))
    ap.add_argument("--kernel", type=int, default=3)
    ap.add_argument("--iters", type=int, default=100)   # windows of 0.1 - 0.4 s at the default shape
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    N, C, K, T, H, W = a.shape
    k, stride, pad = a.kernel, (1, 1, 1), (a.kernel // 2,) * 3
    torch.manual_seed(0)
    x = torch.randn(N, C, T, H, W, device="cuda").bfloat16().float().requires_grad_(True)
    w = (torch.randn(K, C, k, k, k, device="cuda") / (C * k ** 3) ** 0.5).bfloat16().float().requires_grad_(True)
    b = torch.randn(K, device="cuda").requires_grad_(True)
    gy = torch.randn(N, K, T, H, W, device="cuda").bfloat16().float()
    flops = 2.0 * N * T * H * W * K * C * k ** 3
    lines = [f"conv3d A/B: N={N} C={C} K={K} {T}x{H}x{W} kernel {k}^3 stride 1 pad {pad[0]}; device events, "
             f"{a.windows} alternating windows of {a.iters} calls, ms per call: median [min .. max]"]
    results = {}
    for backward in (False, True):
        times = {True: [], False: []}
        for native in (True, False):                      # warm-up of both sides, and their results
            conv_fn.CONV3D_NATIVE[0] = native
            results[native] = run(x, w, b, gy, stride, pad, backward)
            window((x, w, b, gy, stride, pad, backward), 2)
        for _ in range(a.windows):
            for native in (True, False):
                conv_fn.CONV3D_NATIVE[0] = native
                times[native].append(window((x, w, b, gy, stride, pad, backward), a.iters))
        for native in (True, False):
            t = times[native]
            med = statistics.median(t)
            lines.append(f"{'fwd+bwd' if backward else 'fwd    '} {'native ' if native else 'per-tap'} "
                         f"{med:8.3f} [{min(t):8.3f} .. {max(t):8.3f}]  "
                         f"{flops * (3 if backward else 1) / med / 1e9:7.1f} TFLOP/s end to end")
    for name, p, q in zip(("y", "gx", "gw", "gb"), results[True], results[False]):
        lines.append(f"max |native - per-tap| / max |per-tap| of {name}: "
                     f"{((p - q).abs().max() / q.abs().max()).item():.3e}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
