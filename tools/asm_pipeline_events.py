#!/usr/bin/env python3
"""List, in program order, the pipeline events of a kernel in a gfx950 assembly file: LDS-DMA issues, every s_waitcnt
that names vmcnt, barriers, transposing LDS reads, MFMAs, labels and branches. Runs of the same event are folded
("8x dma"). Loops show as a label followed later by a branch back to it.

  hipcc -O3 -std=c++17 --offload-arch=gfx950 -fno-gpu-rdc --cuda-device-only -S -Icsrc csrc/conv_igemm.hip -o x.s
  tools/asm_pipeline_events.py x.s conv_wgrad_glds_kernel [--loops-only]
"""
import re
import subprocess
import sys


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        return dict(zip(names, out.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def classify(ins):
    op = ins.split()[0]
    if op.startswith("global_load_lds") or (op.startswith("buffer_load") and " lds" in ins):
        return "dma"
    if op == "s_waitcnt":
        return ins if "vmcnt" in ins else None
    if op == "s_barrier":
        return "s_barrier"
    if op.startswith("ds_read_b64_tr"):
        return "tr_read"
    if op.startswith("ds_read") or op.startswith("ds_write"):
        return "ds_other"
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith(("global_load", "buffer_load", "scratch_load", "s_load", "s_getpc")):
        return op
    if op.startswith("s_cbranch") or op == "s_branch":
        return ins
    return None


def events(lines):
    ev = []
    for ln in lines:
        s = ln.split(";")[0].strip()
        m = re.match(r"^(\.?[A-Za-z_][\w.$]*):$", s)
        if m:
            ev.append(("label", m.group(1)))
            continue
        if not s or s.startswith("."):
            continue
        c = classify(s)
        if c:
            ev.append(("ev", c))
    return ev


def loops_only(ev):
    """Keep the spans between a label and the last branch back to it."""
    pos = {v: i for i, (k, v) in enumerate(ev) if k == "label"}
    keep = [False] * len(ev)
    edge = set()                         # loop heads and the branches back to them; forward control flow is dropped
    for i, (k, v) in enumerate(ev):
        if k == "ev" and v.startswith(("s_cbranch", "s_branch")):
            tgt = v.split()[-1]
            if tgt in pos and pos[tgt] < i:
                edge.update((pos[tgt], i))
                for j in range(pos[tgt], i + 1):
                    keep[j] = True
    return [e for i, (e, f) in enumerate(zip(ev, keep))
            if f and (i in edge or not (e[0] == "label" or e[1].startswith(("s_cbranch", "s_branch"))))]


def fold(ev):
    out = []
    for k, v in ev:
        if out and out[-1][0] == (k, v) and k == "ev":
            out[-1][1] += 1
        else:
            out.append([(k, v), 1])
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    only = "--loops-only" in sys.argv
    path, pat = args[0], args[1]
    text = open(path).read().splitlines()
    starts = [(i, m.group(1)) for i, l in enumerate(text) for m in [re.match(r"^(_Z\w+):", l)] if m]
    dm = demangle([n for _, n in starts])
    for i, name in starts:
        if pat not in dm[name]:
            continue
        end = next(j for j in range(i, len(text)) if text[j].strip().startswith("s_endpgm"))
        ev = events(text[i + 1:end])
        if only:
            ev = loops_only(ev)
        print(f"== {dm[name]}")
        for (k, v), n in fold(ev):
            if k == "label":
                print(f"{v}:")
            else:
                print(f"    {n}x {v}" if n > 1 else f"    {v}")
        print()


if __name__ == "__main__":
    main()
