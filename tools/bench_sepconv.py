"""A/B timing of depthwise-separable convolution on the GPU: the fused forward (csrc/sepconv.hip) against the
depthwise kernel + pointwise GEMM path, both in this process and this build, alternating windows.

    python tools/bench_sepconv.py [--out FILE]

Times forward alone (no gradient wanted: no mid16 output), then forward + backward, of Xception / MobileNet-like layers
(Cin = Cout, 3 x 3, depth multiplier 1, N = 32) and of the conv-family test's shape, with device events around windows
of calls sized to about --window seconds; prints the median and the range over --rounds rounds per side, the gain and
the larger round-to-round spread, and the largest difference between the two sides' outputs on the same inputs."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bigdl_amd.ops import conv_fn  # noqa: E402

# N, Cin, dm, Cout, H, W, k, stride, pad
SHAPES = [(32, c, 1, c, m, m, 3, s, 1) for c in (128, 256, 728) for m in (56, 28, 14) for s in (1, 2)]
SHAPES.append((2, 8, 2, 24, 10, 10, 3, 1, 1))


def run(t, geo, backward):
    x, wd, wp, b, gy = t
    if not backward:
        with torch.no_grad():
            return (conv_fn.separable_conv2d(x, wd, wp, b, geo[0], geo[1]),)
    y = conv_fn.separable_conv2d(x, wd, wp, b, geo[0], geo[1])
    return (y,) + torch.autograd.grad(y, (x, wd, wp, b), gy)


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
    lines = [f"separable conv A/B: fused (csrc/sepconv.hip) vs split (depthwise kernel + pointwise GEMM); device events, "
             f"{a.rounds} alternating rounds of ~{a.window} s windows, ms per call: median [min .. max]; gain = split / "
             f"fused - 1, spread = the larger (max - min) / median of the two sides"]
    for N, Cin, dm, Cout, H, W, k, s, p in SHAPES:
        torch.manual_seed(0)
        Cmid = Cin * dm
        x = torch.randn(N, Cin, H, W, device="cuda").requires_grad_(True)
        wd = (torch.randn(Cmid, 1, k, k, device="cuda") / k).requires_grad_(True)
        wp = (torch.randn(Cout, Cmid, 1, 1, device="cuda") / Cmid ** 0.5).bfloat16().float().requires_grad_(True)
        b = torch.randn(Cout, device="cuda").requires_grad_(True)
        geo = ((s, s), (p, p))
        gy = None
        name = f"N={N} Cin={Cin} dm={dm} Cout={Cout} {H}x{W} k={k} s={s} p={p}"
        for backward in (False, True):
            mode = "fwd+bwd" if backward else "fwd    "
            out, times, iters = {}, {True: [], False: []}, {}
            for fused in (True, False):                   # warm-up of both sides, their results, and the window size
                conv_fn.set_sepconv_fused(fused)
                if gy is None:
                    gy = torch.randn_like(run((x, wd, wp, b, None), geo, False)[0])
                args = ((x, wd, wp, b, gy), geo, backward)
                out[fused] = run(*args)
                iters[fused] = max(3, min(2000, int(a.window * 1e3 / max(window(args, 3), 1e-3))))
                if fused and conv_fn.last_separable_route() != "fused":
                    break
            else:
                fused = None                              # both sides ran
            if fused is not None:
                lines.append(f"{name} {mode} fused route not taken (geometry outside the kernel's LDS budget): split only")
                continue
            for _ in range(a.rounds):
                for fused in (True, False):
                    conv_fn.set_sepconv_fused(fused)
                    times[fused].append(window(args, iters[fused]))
            med = {f: statistics.median(times[f]) for f in (True, False)}
            spread = max((max(times[f]) - min(times[f])) / med[f] for f in (True, False))
            diff = max(((p_ - q_).abs().max() / q_.abs().max()).item() for p_, q_ in zip(out[True], out[False]))
            lines.append(f"{name} {mode} fused {med[True]:8.3f} [{min(times[True]):8.3f} .. {max(times[True]):8.3f}]  "
                         f"split {med[False]:8.3f} [{min(times[False]):8.3f} .. {max(times[False]):8.3f}]  "
                         f"gain {med[False] / med[True] - 1:+7.1%}  spread {spread:6.1%}  max rel diff {diff:.2e}")
            print(lines[-1], flush=True)
    conv_fn.set_sepconv_fused(None)
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
