#!/usr/bin/env python
"""A/B of the detection post-processing modules with batching off / on (BIGDL_DET_BATCHED 0 / 1: the per-class /
per-level loops against one ``multiclass_nms`` / ``roi_align_levels`` launch, and RegionProposal's per-image, per-level
loop against ``rpn_select``'s one launch per stage, csrc/detection.hip).

  python tools/bench_detection.py              ms per forward of both paths, alternating in one process
  python tools/bench_detection.py --trace      also: kernel launches of one forward per path, each from a
                                               ``rocprofv3 --kernel-trace`` child of its own
  python tools/bench_detection.py --out FILE   append the report to FILE

Every path is bound by the host, so the figure is wall time around a synchronised forward. Each round times
``--iters`` forwards of one path, then of the other; the report gives the median over ``--rounds`` rounds and the
round-to-round spread (max - min). Batching is worth its default for a module only when it wins by more than three
times the larger spread; the verdict column says so.
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

CASES = ["boxpost1", "boxpost2", "pooler7", "pooler14", "ssd", "rpn1", "rpn2", "rpn1stub", "rpn2stub"]
OWN_KERNELS = ("nms_classes_kernel", "roi_align_levels_fwd_kernel", "segmented_topk_maps_kernel",
               "segmented_topk_flat_kernel")


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--cases", default=",".join(CASES))
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--iters", type=int, default=3)
    p.add_argument("--trace", action="store_true")
    p.add_argument("--one", default=None, help="(child) CASE:PATH, two forwards, no timing")
    p.add_argument("--out", default=None)
    return p.parse_args()


def make(case):
    """(run, note): run() is one forward on cuda:0; note describes the workload."""
    import torch

    from bigdl_amd import nn
    from bigdl_amd.utils.table import T, Table

    g = torch.Generator().manual_seed(1)
    dev = torch.device("cuda")
    if case.startswith("boxpost"):
        B, R, C = int(case[len("boxpost"):]), 1000, 81
        logits = torch.randn(B * R, C, generator=g) * 2.0
        deltas = torch.randn(B * R, 4 * C, generator=g) * 0.3
        ctr = torch.randint(0, 24, (B * R,), generator=g)          # proposals cluster around 24 objects
        cx, cy = 100.0 + 200.0 * (ctr % 6).float(), 100.0 + 180.0 * (ctr // 6).float()
        cx, cy = cx + torch.randn(B * R, generator=g) * 15, cy + torch.randn(B * R, generator=g) * 15
        hw = torch.rand(B * R, 2, generator=g) * 60 + 30
        props = torch.stack([cx - hw[:, 0], cy - hw[:, 1], cx + hw[:, 0], cy + hw[:, 1]], 1)
        tab = Table()
        for b in range(B):
            tab[b + 1] = props[b * R:(b + 1) * R].to(dev)
        m = nn.BoxPostProcessor(0.05, 0.5, 100, C).evaluate()
        inp = T(logits.to(dev), deltas.to(dev), tab, torch.tensor([800.0, 1344.0], device=dev))
        passing = (torch.softmax(logits, 1)[:, 1:] > 0.05).sum(0).float().mean() / B
        return (lambda: m.forward(inp)), (f"BoxPostProcessor {B} x {R} proposals x {C} classes, scoreThresh 0.05, "
                                          f"nmsThresh 0.5, maxPerImage 100; {float(passing):.1f} rows per image and "
                                          f"class pass the threshold")
    if case.startswith("pooler"):
        res, R = int(case[len("pooler"):]), 1000
        scales = [0.25, 0.125, 0.0625, 0.03125]
        feats = Table()
        for i, s in enumerate(scales):
            feats[i + 1] = torch.randn(1, 256, int(800 * s), int(1344 * s), generator=g).to(dev)
        side = torch.exp(torch.rand(R, 2, generator=g) * 3.4 + 3.0)        # 20 .. 600 px, log-uniform
        xy = torch.rand(R, 2, generator=g) * torch.tensor([1344.0, 800.0])
        rois = torch.cat([xy - side / 2, xy + side / 2], 1).to(dev)
        m = nn.Pooler(res, scales, 2)
        per_level = torch.bincount(m._levels(rois).cpu(), minlength=4).tolist()
        inp = T(feats, T(rois))
        return (lambda: m.forward(inp)), (f"Pooler {R} rois, 4 levels, 256 channels, resolution {res}, sampling 2; "
                                          f"rois per level {per_level}")
    if case == "ssd":
        B, nP, C = 8, 8732, 21
        prior_xy = torch.rand(nP, 2, generator=g)
        prior_wh = torch.rand(nP, 2, generator=g) * 0.3 + 0.05
        pri = torch.cat([prior_xy - prior_wh / 2, prior_xy + prior_wh / 2], 1).reshape(-1)
        prior = torch.stack([pri, torch.tensor([0.1, 0.1, 0.2, 0.2]).repeat(nP)]).reshape(1, 2, -1)
        loc = torch.randn(B, nP * 4, generator=g) * 0.5
        conf = torch.randn(B, nP, C, generator=g) * 1.5
        conf[:, :, 0] += 6.0                                               # background dominates, as in a real SSD
        cand = (torch.softmax(conf, 2)[:, :, 1:] >= 0.01).sum(1).float().mean()
        m = nn.DetectionOutputSSD(nClasses=C).evaluate()
        inp = T(loc.to(dev), conf.reshape(B, -1).to(dev), prior.to(dev))
        return (lambda: m.forward(inp)), (f"DetectionOutputSSD {B} images x {nP} priors x {C} classes, confThresh 0.01, "
                                          f"nmsTopk 400, keepTopK 200; {float(cand):.0f} candidates per image and "
                                          f"class")
    if case.startswith("rpn"):
        stub = case.endswith("stub")
        B = int(case[len("rpn"):len(case) - (4 if stub else 0)])
        shapes = [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)]      # an 800 x 1344 image at strides 4 .. 64
        m = nn.RegionProposal(256).evaluate().to(dev)
        if stub:
            from bigdl_amd.nn.abstractnn import AbstractModule

            class SliceHead(AbstractModule):                   # objectness / regression are feature channels
                def updateOutput(self, x):
                    return Table(x[:, :3], x[:, 3:15])

            m.head = SliceHead()
            m.modules = [m.head]
        feats = Table()
        for i, (h, w) in enumerate(shapes):
            f = torch.randn(B, 256, h, w, generator=g)
            if stub:
                f[:, 3:15] *= 0.3
            feats[i + 1] = f.to(dev)
        inp = T(feats, torch.tensor([800.0, 1344.0]))
        anchors = sum(3 * h * w for h, w in shapes)
        note = (f"RegionProposal(256) batch {B}, 5 levels 200x336 .. 13x21, {anchors} anchors per image, test mode "
                f"1000 / 1000, nms 0.7" + (", head replaced by a channel-slicing stub" if stub else ""))
        return (lambda: m.forward(inp)), note
    raise ValueError(f"unknown case {case!r}; known: {CASES}")


def forward(run, batched):
    import torch

    from bigdl_amd.ops import detection as D

    D.set_batched(bool(batched))
    try:
        out = run()
        torch.cuda.synchronize()
    finally:
        D.set_batched(None)
    return out


def tensors(out):
    """Every tensor of a module output (Tensor or nested Table), depth first."""
    if hasattr(out, "length"):
        return [t for i in range(out.length()) for t in tensors(out[i + 1])]
    return [out]


def trace_child(case, path):
    """(name, microseconds) of every kernel of a ``--one`` child under rocprofv3 --kernel-trace, in start order: a
    fresh process that builds the inputs and runs the forward of ``path`` twice, so every per-forward count is half
    of what the trace holds."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "det", "--",
               sys.executable, os.path.abspath(__file__), "--one", f"{case}:{path}"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError(f"rocprofv3 child exited {r.returncode}: {r.stderr[-400:]}")
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 wrote no kernel trace")
        rows = []
        for f in files:
            with open(f, newline="") as fh:
                for r in csv.DictReader(fh):
                    rows.append((int(r["Start_Timestamp"]), r["Kernel_Name"],
                                 (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
        rows.sort()
        return [(n, us) for _, n, us in rows]


def main():
    a = parse()
    if a.one is not None:
        case, path = a.one.split(":")
        run, _ = make(case)
        forward(run, int(path))
        forward(run, int(path))
        return
    from bigdl_amd.ops import detection as D

    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    say(f"bench_detection: ms per synchronised forward, {a.rounds} rounds of {a.iters} forwards per path, "
        f"alternating loop / batched in one process; median of the rounds, spread = max - min of the rounds")
    for case in a.cases.split(","):
        run, note = make(case)
        routes, outs = {}, {}
        for path in (0, 1):                                  # warm-up: kernel load, caches, allocator
            outs[path] = [t.clone() for t in tensors(forward(run, path))]
            routes[path] = D.last_route()
        same = len(outs[0]) == len(outs[1]) and all(x.shape == y.shape and bool((x == y).all())
                                                    for x, y in zip(outs[0], outs[1]))
        note += f"; outputs of the two paths {'equal' if same else 'DIFFER'}"
        del outs
        times = {0: [], 1: []}
        for _ in range(a.rounds):
            for path in (0, 1):
                t0 = time.perf_counter()
                for _ in range(a.iters):
                    forward(run, path)
                times[path].append((time.perf_counter() - t0) / a.iters * 1e3)
        med = {p: statistics.median(times[p]) for p in (0, 1)}
        spread = {p: max(times[p]) - min(times[p]) for p in (0, 1)}
        wins = med[0] - med[1] > 3 * max(spread.values())
        say(f"{case}: {note}")
        for p, name in ((0, "loop   "), (1, "batched")):
            say(f"  {name} {med[p]:9.3f} ms  spread {spread[p]:7.3f} ms  rounds "
                + " ".join(f"{t:.3f}" for t in times[p]) + (f"  route {routes[p]}" if p else ""))
        say(f"  loop / batched {med[0] / med[1]:.2f}x; gain {med[0] - med[1]:.3f} ms against 3 x spread "
            f"{3 * max(spread.values()):.3f} ms: batched {'wins' if wins else 'does not win'}")
        if a.trace:
            del run
            try:
                for p, name in ((0, "loop"), (1, "batched")):
                    kernels = trace_child(case, p)
                    names = [n for n, _ in kernels]
                    own = sum(1 for n in names if any(k in n for k in OWN_KERNELS))
                    old = sum(1 for n in names if "nms_mask_kernel" in n or "nms_scan_kernel" in n
                              or "roi_align_fwd_kernel" in n)
                    say(f"  trace {name}: {len(names) // 2} launches per forward (input set-up included), of "
                        f"them {own // 2} nms_classes / roi_align_levels / segmented_topk and {old // 2} nms_mask / "
                        f"nms_scan / roi_align_fwd")
                    for k in OWN_KERNELS[2:]:                  # one workgroup per segment: the longest one sets it
                        us = [t for n, t in kernels if k in n]
                        if us:
                            say(f"    {k}: {len(us) // 2} per forward, last forward "
                                + " ".join(f"{t:.1f}" for t in us[len(us) // 2:]) + " us")
            except (RuntimeError, OSError, KeyError, subprocess.TimeoutExpired) as e:
                say(f"  kernel trace failed: {e}")
    text = "\n".join(lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
