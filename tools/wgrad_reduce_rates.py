"""Bytes, time and GB/s of every weight-gradient split-reduce launch of one ResNet-50 training step (GPU).

Two halves, because a kernel trace has no kernel arguments:

    rocprofv3 --kernel-trace -d DIR -o run -- python tools/wgrad_reduce_rates.py record CALLS.json \
        --steps 5 --warmup 3 --graph 0
    python tools/wgrad_reduce_rates.py table DIR/.../run_results.db CALLS.json [--separate-bias] [--probe-tbs X]

``record`` runs bench.py with the given arguments in this process and logs the geometry of every conv_wgrad call in
call order, with the plan (route, splits) the chooser reports for it. ``table`` lines the reduce dispatches of the trace
up with the calls that launch one (the weight gradients run in call order on one stream), from the end of the run
backwards, and prints one row per launch of one step: median time over the traced steps, floats read
(splits x Ncol x Kdim partials + dW; bias: splits x Ncol + Ncol) and the rate. ``--separate-bias``: the 3x3 and stem
routes sum their bias partials in a launch of their own (builds before the single reduce kernel).
"""
import argparse
import json
import os
import re
import runpy
import sqlite3
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REDUCE = re.compile(r"split_reduce_kernel|wgrad_reduce_kernel|halo_reduce_kernel")


def record(out, bench_args):
    sys.path.insert(0, ROOT)
    from bigdl_amd.ops import native

    C = native.get()
    orig = C.conv_wgrad
    calls = []

    def conv_wgrad(dy, src, dw, dbias, geo, *rest, **kw):
        calls.append((tuple(int(g) for g in geo), dbias is not None))
        return orig(dy, src, dw, dbias, geo, *rest, **kw)

    C.conv_wgrad = conv_wgrad
    sys.argv = [os.path.join(ROOT, "bench.py")] + bench_args
    try:
        runpy.run_path(sys.argv[0], run_name="__main__")
    finally:
        C.conv_wgrad = orig
        plans = {k: (C.conv_wgrad_plan_name(list(k[0]), k[1]), list(C.conv_wgrad_plan_info(list(k[0]), k[1])))
                 for k in set(calls)}
        with open(out, "w") as f:
            json.dump([{"geo": g, "bias": b, "route": plans[(g, b)][0], "plan": plans[(g, b)][1]} for g, b in calls], f)


def launches_of(call, separate_bias):
    """[(what, splits, floats read)] of the reduce launches one conv_wgrad call makes."""
    geo, bias, route, plan = call["geo"], call["bias"], call["route"], call["plan"]
    ncol, kdim = geo[15], geo[16]
    splits, ws = plan[0], plan[1]
    if ws <= 0:
        return []
    if route == "stem":
        splits = ws // (ncol * kdim + ncol)
    if splits <= 1:
        return []
    dw = (splits + 1) * ncol * kdim
    db = (splits + 1) * ncol if bias and route in ("stem", "halo") else 0
    if db and separate_bias:
        return [("dW", splits, dw), ("dbias", splits, db)]
    return [("dW+dbias" if db else "dW", splits, dw + db)]


def table(db, calls_path, separate_bias, probe_tbs):
    with open(calls_path) as f:
        calls = json.load(f)
    c = sqlite3.connect(db)
    cols = [r[1] for r in c.execute("pragma table_info(kernels)")]
    name_col = "kernel_name" if "kernel_name" in cols else "name"
    disp = [(n, e - s) for n, s, e in c.execute(f"select {name_col}, start, end from kernels order by start")
            if REDUCE.search(n)]
    # one step = the shortest period of the call log's tail
    keys = [(tuple(x["geo"]), x["bias"]) for x in calls]
    per = next(p for p in range(1, len(keys) + 1) if keys[-p:] == keys[-2 * p:-p])
    step = calls[-per:]
    rows = [(ci, lt) for ci, call in enumerate(step) for lt in launches_of(call, separate_bias)]
    steps = min(len(disp) // len(rows), len(keys) // per)
    assert steps >= 1, (len(disp), len(rows))
    if len(disp) % len(rows):
        print(f"# WARNING: {len(disp)} reduce dispatches are no multiple of {len(rows)} expected per step")
    tail = disp[len(disp) - steps * len(rows):]
    print(f"# {len(rows)} reduce launches per step over {per} conv_wgrad calls; median of {steps} traced steps; "
          f"{len(disp)} reduce dispatches in the trace")
    if probe_tbs:
        print(f"# read rate of a trivial kernel at 32 MiB on the same box (tools/hbm_probe.py --mib 32): "
              f"{probe_tbs:.2f} TB/s")
    print(f"# {'layer (backward order)':44s} {'route':10s} {'what':9s} {'splits':>6s} {'MB read':>8s} {'us':>8s} "
          f"{'GB/s':>7s}" + (f" {'of probe':>8s}" if probe_tbs else ""))
    tot_us = tot_b = 0.0
    for ri, (ci, (what, splits, floats)) in enumerate(rows):
        ts = [tail[s * len(rows) + ri] for s in range(steps)]
        names = {REDUCE.search(n).group(0) for n, _ in ts}
        us = statistics.median(d for _, d in ts) / 1e3
        g = step[ci]["geo"]
        layer = f"{ci:2d} {g[6]}x{g[7]}/s{g[8]} {g[16] // (g[6] * g[7])}->{g[15]} at {g[1]}x{g[2]} out {g[4]}x{g[5]}"
        gbs = floats * 4 / us / 1e3
        tot_us += us
        tot_b += floats * 4
        print(f"  {layer:44s} {step[ci]['route']:10s} {what:9s} {splits:6d} {floats * 4 / 1e6:8.2f} {us:8.1f} {gbs:7.0f}"
              + (f" {100 * gbs / (probe_tbs * 1e3):7.0f}%" if probe_tbs else "") + f"  {'/'.join(sorted(names))}")
    print(f"# total: {len(rows)} launches, {tot_b / 1e6:.1f} MB, {tot_us / 1e3:.3f} ms per step, "
          f"{tot_b / tot_us / 1e3:.0f} GB/s overall")


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    r = sub.add_parser("record")
    r.add_argument("out")
    t = sub.add_parser("table")
    t.add_argument("db")
    t.add_argument("calls")
    t.add_argument("--separate-bias", action="store_true")
    t.add_argument("--probe-tbs", type=float, default=0.0)
    a, rest = ap.parse_known_args()
    if a.mode == "record":
        record(a.out, rest)
    else:
        table(a.db, a.calls, a.separate_bias, a.probe_tbs)


if __name__ == "__main__":
    main()
