"""A/B of the two attention dQ routes (csrc/attention.hip): forward + backward of ops.flash_attention with dQ through
fp32 atomics over key blocks ("atomic", the default) against the ordered kernel ("ordered": one workgroup per query
block, key blocks in order, S / P / dP recomputed once more; what deterministic mode runs).

Both routes run in one process on the same random inputs, interleaved round by round; per shape the median of three
rounds and their spread are printed, each round the mean over --iters calls between device events after a warm-up.

    python tools/attn_dq_ab.py [--iters 20] [--out profiles/attn_dq_ordered_ab.txt]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bigdl_amd.ops import flash_attention as fa  # noqa: E402

# (B*H, L, D, causal): Transformer self-attention shapes, 256 (batch x heads) of 64-wide heads
SHAPES = [(256, 512, 64, False), (256, 512, 64, True), (256, 2048, 64, False), (256, 2048, 64, True),
          (64, 1024, 128, True)]
ROUNDS = 3


def one_round(q, k, v, do, causal, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        for t in (q, k, v):
            t.grad = None
        fa.flash_attention(q, k, v, None, causal).backward(do)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def measure(BH, L, D, causal, iters):
    g = torch.Generator(device="cpu").manual_seed(L + D)
    q = (torch.randn(1, BH, L, D, generator=g) * D ** -0.5).cuda().requires_grad_(True)
    k = torch.randn(1, BH, L, D, generator=g).cuda().requires_grad_(True)
    v = torch.randn(1, BH, L, D, generator=g).cuda().requires_grad_(True)
    do = torch.randn(1, BH, L, D, generator=g).cuda()
    ms = {"atomic": [], "ordered": []}
    dq = {}
    try:
        for mode in ms:                                  # warm-up, and the two routes' dQ on the same inputs
            fa.set_dq_mode(mode)
            one_round(q, k, v, do, causal, 2)
            dq[mode] = q.grad.clone()
        for _ in range(ROUNDS):
            for mode in ms:
                fa.set_dq_mode(mode)
                ms[mode].append(one_round(q, k, v, do, causal, iters))
    finally:
        fa.set_dq_mode(None)
    diff = (dq["atomic"] - dq["ordered"]).abs().max().item() / dq["atomic"].abs().max().item()
    return {m: sorted(v) for m, v in ms.items()}, diff


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [f"attention forward + backward, dQ atomic vs ordered; ms per call, median of {ROUNDS} interleaved rounds "
             f"[min .. max], {a.iters} calls per round; {torch.cuda.get_device_properties(0).gcnArchName}"]
    for BH, L, D, causal in SHAPES:
        ms, diff = measure(BH, L, D, causal, a.iters)
        at, od = ms["atomic"], ms["ordered"]
        lines.append(f"B*H={BH} L={L} D={D} causal={int(causal)}: atomic {at[1]:.3f} [{at[0]:.3f} .. {at[2]:.3f}]  "
                     f"ordered {od[1]:.3f} [{od[0]:.3f} .. {od[2]:.3f}]  ordered/atomic {od[1] / at[1]:.3f}  "
                     f"max |dq_atomic - dq_ordered| / max |dq| {diff:.2e}")
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
