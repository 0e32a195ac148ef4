#!/usr/bin/env python
"""A/B of the LARS end-of-step path: the fused route (csrc/lars.hip: norms, finish, update = three launches for all
layers) against the per-layer loop (``ops.lars.set_fused`` on / off), on ResNet-50 with one LarsSGD per layer
(``LarsSGD.createOptimForModule``).

  python tools/bench_lars.py                  tail and whole-step times of both routes, alternating in one process
  python tools/bench_lars.py --trace          also: kernel launches per tail / per step of each route, each from
                                              ``rocprofv3 --kernel-trace --stats`` children of their own
  python tools/bench_lars.py --out FILE --trace-out FILE     append the reports to files

The model's layer regularizers are removed and their 1e-4 goes into LarsSGD's weightDecay (the reference's LARS
recipe): with folded regularizers a TrainStep keeps LARS on the per-layer route (README "Fused LARS").

(a) tail: ``apply_processors`` + ``optimize_pieces`` on fixed gradients, device events around ``--reps`` repetitions;
(b) whole steps: wall time around ``--steps`` synchronised ``TrainStep.step`` calls at ``--batch``.
Each round times one route, then the other; the report gives the median over ``--rounds`` rounds and the
round-to-round spread (max - min). Fused is worth being the default only when the whole-step gain exceeds three times
the larger spread. The update kernel's bytes/s stand next to sgd4_kernel's over the same element count (both move 22
bytes per element: w, g, momentum in; w, momentum, the bf16 shadow out).
"""
import argparse
import csv
import glob
import os
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

ROUTES = ((0, "loop "), (1, "fused"))


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--depth", type=int, default=50)
    p.add_argument("--reps", type=int, default=200)
    p.add_argument("--steps", type=int, default=8)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--trace", action="store_true")
    p.add_argument("--one", default=None, help="(child) ROUTE:KIND:N, N tails or steps after two warm ones, no timing")
    p.add_argument("--out", default=None)
    p.add_argument("--trace-out", default=None)
    return p.parse_args()


def build(route, depth):
    """A TrainStep over ResNet-``depth`` with one LarsSGD per layer, built with the switch at ``route``."""
    import torch

    from bigdl_amd import nn
    from bigdl_amd.models.resnet import DatasetType, ResNet
    from bigdl_amd.ops import lars
    from bigdl_amd.optim.methods import LarsSGD
    from bigdl_amd.optim.sgd import Poly
    from bigdl_amd.optim.train_step import TrainStep
    from bigdl_amd.utils.random_generator import RNG

    RNG.setSeed(1234)
    model = ResNet(1000, depth, dataSet=DatasetType.ImageNet)
    for m in model.flattened_layers():
        if getattr(m, "wRegularizer", None) is not None or getattr(m, "bRegularizer", None) is not None:
            m.wRegularizer = m.bRegularizer = None
    methods = LarsSGD.createOptimForModule(model, Poly(2.0, 1000000), trust=1e-3, learningRate=1e-3,
                                           weightDecay=1e-4, momentum=0.9)
    lars.set_fused(bool(route))
    try:
        step = TrainStep(model, nn.CrossEntropyCriterion(), methods, device=torch.device("cuda"))
    finally:
        lars.set_fused(None)
    assert (step.lars_plan is not None) == bool(route), "the switch did not choose the route"
    g = torch.Generator(device="cuda").manual_seed(7)
    step.g.copy_(1e-3 * torch.randn(step.g.numel(), device="cuda", generator=g))
    return step


def tail(step):
    step.apply_processors()
    step.optimize_pieces(0.0)


def batch(step, B):
    import torch

    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(B, 3, 224, 224, device="cuda", generator=g)
    y = torch.randint(1, 1001, (B,), device="cuda", generator=g).float()
    return x, y


def time_tail(step, reps):
    """(device ms, wall ms) per tail."""
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        tail(step)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, (time.perf_counter() - t0) / reps * 1e3


def time_steps(step, x, y, n):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        step.step(x, y)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def kernel_rates(step, reps):
    """GB/s of lars_update_kernel over every LARS element and of sgd4_kernel (momentum, bf16 shadow) over as many."""
    import torch

    from bigdl_amd.ops import native

    lp = step.lars_plan
    n = sum(hi - lo for lo, hi, _ in lp.spans)
    C = native.get()
    w = torch.zeros(n, device="cuda")
    g = torch.full((n,), 1e-3, device="cuda")
    mom = torch.zeros(n, device="cuda")
    w16 = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    WD = step._lars_processor.weightDecay

    def lars_update():
        lp.update(step.w, step.g, step.w16, WD)

    def sgd():
        C.sgd_step(w, g, mom, w16, 1e-3, 1e-4, 0.9, 0.0, False, False)

    out = {}
    lp.norms(step.w, step.g)
    for name, fn in (("lars_update_kernel", lars_update), ("sgd4_kernel", sgd)):
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / reps
        out[name] = (ms, 22.0 * n / (ms * 1e-3) / 1e9)
    return n, out


def trace_child(route, kind, n, a):
    """Kernel names of a ``--one`` child under rocprofv3 --kernel-trace --stats, in start order."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "lars", "--",
               sys.executable, os.path.abspath(__file__), "--one", f"{route}:{kind}:{n}", "--batch", str(a.batch),
               "--depth", str(a.depth)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError(f"rocprofv3 child exited {r.returncode}: {r.stderr[-400:]}")
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 wrote no kernel trace")
        rows = []
        for f in files:
            with open(f, newline="") as fh:
                for r in csv.DictReader(fh):
                    rows.append((int(r["Start_Timestamp"]), r["Kernel_Name"]))
        rows.sort()
        return [n for _, n in rows]


def launches(route, kind, a):
    """Launches per tail / step: the difference of two children that differ by four repetitions."""
    few, many = trace_child(route, kind, 1, a), trace_child(route, kind, 5, a)
    own = sum(1 for k in many if "lars_" in k) - sum(1 for k in few if "lars_" in k)
    return (len(many) - len(few)) / 4.0, own / 4.0


def main():
    a = parse()
    if a.one is not None:
        import torch

        route, kind, n = a.one.split(":")
        step = build(int(route), a.depth)
        run = (lambda: tail(step)) if kind == "tail" else None
        if run is None:
            x, y = batch(step, a.batch)
            run = lambda: step.step(x, y)  # noqa: E731
        for _ in range(2 + int(n)):
            run()
        torch.cuda.synchronize()
        return
    import torch

    from bigdl_amd.ops import lars

    lines, tlines = [], []

    def say(line, to=lines):
        to.append(line)
        print(line, flush=True)

    steps = {r: build(r, a.depth) for r, _ in ROUTES}
    nl = len(steps[1].lars_plan.methods)
    say(f"bench_lars: ResNet-{a.depth}, {nl} LarsSGD pieces, {steps[1].lars_plan.nchunks} chunks, batch {a.batch}; "
        f"{a.rounds} rounds per route, alternating loop / fused in one process; median of the rounds, spread = max - "
        f"min of the rounds")
    routes = {}
    for r, _ in ROUTES:                                    # warm-up: kernel load, allocator, state buffers
        for _ in range(3):
            tail(steps[r])
        routes[r] = lars.last_route()
    torch.cuda.synchronize()
    dev, wall = {0: [], 1: []}, {0: [], 1: []}
    for _ in range(a.rounds):
        for r, _ in ROUTES:
            d, w = time_tail(steps[r], a.reps)
            dev[r].append(d)
            wall[r].append(w)
    say(f"(a) tail alone: apply_processors + optimize_pieces on fixed gradients, {a.reps} repetitions per round")
    for r, name in ROUTES:
        say(f"  {name} device {statistics.median(dev[r]):8.3f} ms  spread {max(dev[r]) - min(dev[r]):6.3f} ms | wall "
            f"{statistics.median(wall[r]):8.3f} ms  spread {max(wall[r]) - min(wall[r]):6.3f} ms  route {routes[r]}")
    say(f"  loop / fused: device {statistics.median(dev[0]) / statistics.median(dev[1]):.1f}x, wall "
        f"{statistics.median(wall[0]) / statistics.median(wall[1]):.1f}x")
    x, y = batch(steps[0], a.batch)
    for r, _ in ROUTES:
        for _ in range(3):
            steps[r].step(x, y)
    whole = {0: [], 1: []}
    for _ in range(a.rounds):
        for r, _ in ROUTES:
            whole[r].append(time_steps(steps[r], x, y, a.steps))
    med = {r: statistics.median(whole[r]) for r in whole}
    spread = {r: max(whole[r]) - min(whole[r]) for r in whole}
    say(f"(b) whole steps: {a.steps} synchronised TrainStep.step calls per round")
    for r, name in ROUTES:
        say(f"  {name} {med[r]:9.3f} ms/step  spread {spread[r]:7.3f} ms  rounds "
            + " ".join(f"{t:.3f}" for t in whole[r]))
    gain, need = med[0] - med[1], 3 * max(spread.values())
    say(f"  gain {gain:.3f} ms/step against 3 x spread {need:.3f} ms: fused "
        f"{'wins: the default' if gain > need else 'does not win by that margin: opt-in'}")
    n, rates = kernel_rates(steps[1], a.reps)
    say(f"(c) update kernels over {n} elements, 22 bytes per element, {a.reps} launches each")
    for k, (ms, gbs) in rates.items():
        say(f"  {k:18s} {ms * 1e3:8.1f} us  {gbs:7.0f} GB/s")
    say(f"  lars_update_kernel / sgd4_kernel rate: {rates['lars_update_kernel'][1] / rates['sgd4_kernel'][1]:.2f}")
    if a.trace:
        del steps
        torch.cuda.empty_cache()
        say(f"bench_lars --trace: ResNet-{a.depth}, batch {a.batch}; kernel launches from rocprofv3 --kernel-trace "
            f"--stats children (two runs that differ by four repetitions, difference / 4)", tlines)
        try:
            for kind in ("tail", "step"):
                for r, name in ROUTES:
                    total, own = launches(r, kind, a)
                    say(f"  {kind} {name}: {total:.1f} launches, of them {own:.1f} lars_* kernels", tlines)
        except (RuntimeError, OSError, KeyError, subprocess.TimeoutExpired) as e:
            say(f"  kernel trace failed: {e}", tlines)
    for path, ls in ((a.out, lines), (a.trace_out, tlines)):
        if path and ls:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "a") as fh:
                fh.write("\n".join(ls) + "\n")


if __name__ == "__main__":
    main()
