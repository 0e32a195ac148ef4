#!/usr/bin/env python
"""A/B of Transformer beam-search prediction (``tr.forward(src)``) with native incremental decoding off / on
(BIGDL_DECODE_NATIVE 0 / 1: the Table path against nn/transformer.py _DecodeState on csrc/attn_decode.hip).

  python tools/bench_decode.py                 tokens/s of both variants, alternating in one process, medians
  python tools/bench_decode.py --trace         also: kernel launches per decode step and attn_decode's achieved
                                               bytes/s, each from a ``rocprofv3 --kernel-trace`` child of its own
  python tools/bench_decode.py --out FILE      append the report to FILE

tokens/s counts the tokens of the returned best sequences (batch x decoded steps). The end-of-sentence id is set
outside the vocabulary so every run decodes maxDecodeLength steps.
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


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--vocab", type=int, default=8192)
    p.add_argument("--hidden", type=int, default=512)
    p.add_argument("--heads", type=int, default=8)
    p.add_argument("--filter", type=int, default=2048)
    p.add_argument("--layers", type=int, default=6)
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--beam", type=int, default=4)
    p.add_argument("--src-len", type=int, default=32)
    p.add_argument("--max-len", type=int, default=64)
    p.add_argument("--runs", type=int, default=3)
    p.add_argument("--trace", action="store_true")
    p.add_argument("--one", type=int, default=None, help="(child) one forward of this variant, no timing")
    p.add_argument("--out", default=None)
    return p.parse_args()


def make(a, max_len):
    import torch

    from bigdl_amd import nn
    from bigdl_amd.utils.random_generator import RNG

    RNG.setSeed(1)
    torch.manual_seed(1)
    bs = nn.SequenceBeamSearch(a.vocab, a.beam, 0.6, max_len, float(a.vocab + 5), 0.0, a.layers, a.hidden)
    tr = nn.Transformer(a.vocab, a.hidden, a.heads, a.filter, a.layers, 1.0, 1.0, 1.0, withShareWeightsLinear=True,
                        transformerType=nn.Translation, beamSearch=bs).evaluate()
    tr.embedding.weight.data.mul_(0.1)
    src = torch.randint(3, a.vocab + 1, (a.batch, a.src_len)).float()
    for b in range(a.batch):
        src[b, a.src_len - b % 3:] = 0
    dev = torch.device("cuda")
    return tr.to(dev), src.to(dev)


def forward(tr, src, variant):
    import torch

    from bigdl_amd.ops import attention

    attention.set_decode_native(bool(variant))
    try:
        out = tr.forward(src)
        torch.cuda.synchronize()
    finally:
        attention.set_decode_native(None)
    return out


def trace_child(a, variant, max_len):
    """One forward of ``variant`` under rocprofv3 --kernel-trace in a fresh process: [(kernel name, ns)]."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "decode", "--",
               sys.executable, os.path.abspath(__file__), "--one", str(variant), "--max-len", str(max_len)]
        for k in ("vocab", "hidden", "heads", "filter", "layers", "batch", "beam"):
            cmd += [f"--{k}", str(getattr(a, k))]
        cmd += ["--src-len", str(a.src_len)]
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
                                 int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
        rows.sort()
        return [(n, ns) for _, n, ns in rows]


def trace_report(a, lines):
    short = max(2, a.max_len // 2)
    for variant in (0, 1):
        full, half = trace_child(a, variant, a.max_len), trace_child(a, variant, short)
        per_step = (len(full) - len(half)) / float(a.max_len - short)
        lines.append(f"variant {variant}: {len(full)} launches at {a.max_len} steps, {len(half)} at {short} steps: "
                     f"{per_step:.1f} launches per decode step")
        if variant != 1:
            continue
        calls = [ns for n, ns in full if "attn_decode_kernel" in n]
        if len(calls) != 2 * a.layers * a.max_len:
            lines.append(f"attn_decode: {len(calls)} calls in the trace, expected {2 * a.layers * a.max_len}")
            continue
        N = a.batch * a.beam
        self_b = self_ns = enc_b = enc_ns = 0
        for c, ns in enumerate(calls):                   # per step and layer: self-attention, then encoder-decoder
            step, enc = c // (2 * a.layers), c % 2 == 1
            if enc:                                      # K and V of the B sentences, shared by their beams
                enc_b += a.batch * a.src_len * a.hidden * 2 * 2
                enc_ns += ns
            else:
                self_b += N * (step + 1) * a.hidden * 2 * 2
                self_ns += ns
        lines.append(f"attn_decode self-attention: {self_b / 1e6:.1f} MB of K/V to read in {self_ns / 1e3:.0f} us "
                     f"over {len(calls) // 2} calls: {self_b / self_ns:.1f} GB/s, {2 * self_ns / len(calls) / 1e3:.1f} "
                     f"us per call")
        lines.append(f"attn_decode encoder-decoder: {enc_b / 1e6:.1f} MB of distinct K/V in {enc_ns / 1e3:.0f} us "
                     f"over {len(calls) // 2} calls: {enc_b / enc_ns:.1f} GB/s ({a.beam} beams read each row), "
                     f"{2 * enc_ns / len(calls) / 1e3:.1f} us per call")


def main():
    a = parse()
    if a.one is not None:
        tr, src = make(a, a.max_len)
        forward(tr, src, a.one)
        return
    tr, src = make(a, a.max_len)
    for variant in (0, 1):                               # warm-up: kernel selection, caches, allocator
        forward(tr, src, variant)
    times = {0: [], 1: []}
    for _ in range(a.runs):
        for variant in (0, 1):
            t0 = time.perf_counter()
            out = forward(tr, src, variant)
            times[variant].append(time.perf_counter() - t0)
            assert out[1].shape == (a.batch, a.max_len), out[1].shape
    tokens = a.batch * a.max_len
    lines = [f"bench_decode: vocab {a.vocab} hidden {a.hidden} heads {a.heads} filter {a.filter} layers {a.layers} "
             f"batch {a.batch} beam {a.beam} src-len {a.src_len} maxDecodeLength {a.max_len}; {a.runs} runs each, "
             f"alternating, medians"]
    med = {}
    for variant in (0, 1):
        med[variant] = statistics.median(times[variant])
        runs = " ".join(f"{t * 1e3:.1f}" for t in times[variant])
        lines.append(f"BIGDL_DECODE_NATIVE={variant}: {tokens / med[variant]:.0f} tokens/s "
                     f"(median {med[variant] * 1e3:.1f} ms per forward; runs {runs} ms)")
    lines.append(f"native / table: {med[0] / med[1]:.2f}x")
    if a.trace:
        del tr, src
        try:
            trace_report(a, lines)
        except (RuntimeError, OSError, KeyError, subprocess.TimeoutExpired) as e:
            lines.append(f"kernel trace failed: {e}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
