"""Deterministic-mode check on the GPU (bigdl.deterministic): ResNet-20 (CIFAR-10 shape, BatchNorm, SGD + momentum)
trained for --iters iterations twice from the same seed must end with bitwise-equal weights; the same two runs without
the mode show how far the default (fp32-atomic) reductions drift. Also times a ResNet-50 batch-256 step in both modes
(--r50) to record the mode's cost. --transformer does the same for a Transformer LM step (ordered attention dQ,
LayerNorm parameter gradients and embedding gradient in fixed order): bitwise repeat in the mode, drift of two
default-mode runs, and the mode's cost on a larger LM step.

    python tools/det_check.py [--iters 10] [--r50] [--transformer]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bigdl_amd.ops import native  # noqa: E402


def run(iters, det, depth=20, batch=128, classes=10, image=32, dataset="CIFAR10", seed=3):
    from bigdl_amd import nn
    from bigdl_amd.models.resnet import DatasetType, ResNet
    from bigdl_amd.optim.sgd import SGD
    from bigdl_amd.optim.train_step import TrainStep
    from bigdl_amd.utils.random_generator import RNG

    native.set_deterministic(det)
    RNG.setSeed(seed)
    torch.manual_seed(seed)
    dev = torch.device("cuda")
    model = ResNet(classes, depth, dataSet=getattr(DatasetType, dataset))
    step = TrainStep(model, nn.CrossEntropyCriterion(), SGD(learningRate=0.1, momentum=0.9, dampening=0.0,
                                                             weightDecay=1e-4), device=dev)
    g = torch.Generator(device="cpu").manual_seed(seed)
    xs = [torch.randn(batch, 3, image, image, generator=g).to(dev) for _ in range(2)]
    ys = [torch.randint(1, classes + 1, (batch,), generator=g).float().to(dev) for _ in range(2)]
    torch.cuda.synchronize()
    t0 = None
    for it in range(iters):
        if it == 2:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        step.step(xs[it % 2], ys[it % 2])
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / max(1, iters - 2) if t0 is not None else float("nan")
    step.flush() if hasattr(step, "flush") else None
    w = step.w[:step.total].detach().clone()
    native.set_deterministic(False)
    return w, ms


def transformer_lm(vocab=100, hidden=128, heads=2, filt=256, layers=2, keep=0.9):
    """nn.Transformer as a language model with the shared embedding as its output layer; all three dropouts drop
    1 - keep. Returns (model, criterion): the criterion of the PTB Transformer trainer (examples/ptb_word_lm.py)."""
    from bigdl_amd import nn

    model = nn.Transformer(vocab, hidden, heads, filt, layers, keep, keep, keep, withShareWeightsLinear=True)
    return model, nn.TimeDistributedCriterion(nn.CrossEntropyCriterion(), sizeAverage=False, dimension=2)


def lm_batch(vocab, batch, length, seed, pad_from=None):
    """ids [batch, length] in 1..vocab with a padded (id 0) tail on every other row, and labels in 1..vocab."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randint(1, vocab + 1, (batch, length), generator=g).float()
    pad_from = length - length // 8 if pad_from is None else pad_from
    x[::2, pad_from:] = 0.0
    y = torch.randint(1, vocab + 1, (batch, length), generator=g).float()
    return x, y


def run_transformer(iters, det, base=None, vocab=100, hidden=128, heads=2, filt=256, layers=2, batch=4, length=130,
                    seed=3, optim="adam"):
    """Train a copy of ``base`` (or a fresh transformer_lm) for ``iters`` TrainStep iterations from ``seed``.
    Returns (weights, ms per step over the iterations after the first two)."""
    import copy

    from bigdl_amd.optim.methods import Adam
    from bigdl_amd.optim.sgd import SGD
    from bigdl_amd.optim.train_step import TrainStep
    from bigdl_amd.utils.random_generator import RNG

    saved = native.deterministic()
    native.set_deterministic(det)
    try:
        RNG.setSeed(seed)
        torch.manual_seed(seed)
        dev = torch.device("cuda")
        model, crit = base if base is not None else transformer_lm(vocab, hidden, heads, filt, layers)
        model, crit = copy.deepcopy(model), copy.deepcopy(crit)
        method = Adam(learningRate=1e-3) if optim == "adam" else SGD(learningRate=0.05, momentum=0.9, dampening=0.0)
        step = TrainStep(model, crit, method, device=dev)
        data = [tuple(t.to(dev) for t in lm_batch(vocab, batch, length, seed + i)) for i in range(2)]
        torch.cuda.synchronize()
        t0 = None
        for it in range(iters):
            if it == 2:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            step.step(*data[it % 2])
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / max(1, iters - 2) if t0 is not None and iters > 2 else float("nan")
        step.flush()
        return step.w[:step.total].detach().clone(), ms
    finally:
        native.set_deterministic(saved)


def transformer_report(iters):
    base = transformer_lm()
    for det in (True, False):
        w1, _ = run_transformer(iters, det, base)
        w2, _ = run_transformer(iters, det, base)
        print(f"Transformer LM (vocab 100, hidden 128, 2 layers, 4 x 130 tokens) x{iters} iterations, "
              f"deterministic={det}: bitwise equal {torch.equal(w1, w2)}, max |dw| {(w1 - w2).abs().max().item():.3e}",
              flush=True)
    # cost: a PTB-sized LM step (vocab 10000, hidden 512, 8 heads of 64, 4 layers, 32 x 512 tokens), modes
    # interleaved, three runs each; median and spread
    big = dict(vocab=10000, hidden=512, heads=8, filt=2048, layers=4, batch=32, length=512)
    base = transformer_lm(big["vocab"], big["hidden"], big["heads"], big["filt"], big["layers"])
    ms = {False: [], True: []}
    for _ in range(3):
        for det in (False, True):
            ms[det].append(run_transformer(12, det, base, **big)[1])
    for det in (False, True):
        v = sorted(ms[det])
        print(f"Transformer LM step (vocab 10000, hidden 512, 8 heads, 4 layers, 32 x 512 tokens), "
              f"deterministic={det}: median {v[1]:.2f} ms/step (min {v[0]:.2f}, max {v[2]:.2f}; 10 timed steps x 3 "
              f"interleaved runs)", flush=True)
    print(f"deterministic / default = {sorted(ms[True])[1] / sorted(ms[False])[1]:.3f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--r50", action="store_true")
    ap.add_argument("--transformer", action="store_true")
    a = ap.parse_args()
    if a.transformer:
        transformer_report(a.iters)
        return
    for det in (True, False):
        w1, _ = run(a.iters, det)
        w2, _ = run(a.iters, det)
        d = (w1 - w2).abs().max().item()
        print(f"ResNet-20 x{a.iters} iterations, deterministic={det}: bitwise equal {torch.equal(w1, w2)}, "
              f"max |dw| {d:.3e}", flush=True)
    if a.r50:
        for det in (False, True, False, True):
            _, ms = run(8, det, depth=50, batch=256, classes=1000, image=224, dataset="ImageNet")
            print(f"ResNet-50 b256 step, deterministic={det}: {ms:.2f} ms/step (eager, 6 timed)", flush=True)


if __name__ == "__main__":
    main()
