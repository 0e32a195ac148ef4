"""Deterministic mode on the CPU engine: toggling it changes no result of LookupTable, LayerNormalization or
ops.attention.attention and reaches no native kernel. Also the position-order emulation that
tests/test_det_reductions_gpu.py holds the GPU embedding gradient to, checked here against an fp64 index_add, and
the attention dQ route switch as the native module reads it at start-up."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def embedding_emulation(gout, keys, gw0, scale):
    """The deterministic embedding gradient's stated order in plain fp32 on the CPU: for every weight row r,
    s = g[first position]; s += g[next position] ... in ascending token position, then gW[r] += scale * s once.
    gout [N, D] fp32, keys [N] int64 (negative: skipped), gw0 [rows, D] fp32. Returns the new gW."""
    assert gout.dtype == torch.float32 and gw0.dtype == torch.float32
    out = gw0.clone()
    for r in sorted(set(keys[keys >= 0].tolist())):
        pos = (keys == r).nonzero().flatten().tolist()   # ascending
        s = gout[pos[0]].clone()
        for p in pos[1:]:
            s += gout[p]
        out[r] += scale * s
    return out


def test_emulation_agrees_with_fp64_index_add():
    """n fp32 additions per column: within (n + 1) 2^-24 (|start| + sum |terms|) of the exact sum."""
    g = torch.Generator().manual_seed(1)
    n, rows, D = 4096, 50, 70
    live = torch.tensor([3, 7, 8, 20, 21, 33, 49])
    keys = live[torch.randint(0, 7, (n,), generator=g)]
    keys[torch.randperm(n, generator=g)[:300]] = -1
    gout, gw0 = torch.randn(n, D, generator=g), torch.randn(rows, D, generator=g)
    for scale in (1.0, 0.5):
        got = embedding_emulation(gout, keys, gw0, scale)
        keep = keys >= 0
        exact = gw0.double().index_add(0, keys[keep], gout[keep].double() * scale)
        mag = gw0.double().abs().index_add(0, keys[keep], gout[keep].double().abs() * scale)
        cnt = torch.bincount(keys[keep], minlength=rows).max().item()
        assert ((got.double() - exact).abs() <= (cnt + 1) * 2.0 ** -24 * mag).all()
        dead = [r for r in range(rows) if r not in live.tolist()]
        assert torch.equal(got[dead], gw0[dead])


def _cpu_results():
    from bigdl_amd import nn
    from bigdl_amd.ops.attention import attention
    from bigdl_amd.utils.random_generator import RNG

    RNG.setSeed(5)
    torch.manual_seed(5)
    out = []
    lt = nn.LookupTable(20, 6, paddingValue=3.0, maskZero=True)
    ids = torch.randint(0, 21, (4, 9)).float()
    y = lt.forward(ids)
    lt.zeroGradParameters()
    lt.backward(ids, torch.randn(4, 9, 6))
    out += [y.clone(), lt.gradWeight.clone()]
    ln = nn.LayerNormalization(6)
    x = torch.randn(4, 9, 6)
    y = ln.forward(x)
    ln.zeroGradParameters()
    gi = ln.backward(x, torch.randn(4, 9, 6))
    out += [y.clone(), gi.clone(), ln.gradWeight.clone(), ln.gradBias.clone()]
    q, k, v = (torch.randn(2, 2, 5, 32).requires_grad_(True) for _ in range(3))
    bias = torch.zeros(2, 1, 1, 5)
    bias[..., 4:] = -1e9
    o = attention(q, k, v, bias)
    o.backward(torch.randn_like(o))
    out += [o.detach().clone(), q.grad.clone(), k.grad.clone(), v.grad.clone()]
    return out


def test_cpu_engine_ignores_the_mode(monkeypatch):
    from bigdl_amd.ops import native

    def boom():
        raise AssertionError("native call on the CPU engine")

    saved = native.deterministic()
    try:
        monkeypatch.setattr(native, "get", boom)
        native.set_deterministic(False)
        off = _cpu_results()
        native.set_deterministic(True)
        on = _cpu_results()
    finally:
        native.set_deterministic(saved)
    assert len(on) == len(off) == 10
    for a, b in zip(on, off):
        assert torch.isfinite(a).all() and torch.equal(a, b)


@pytest.mark.parametrize("env,det,want", [("", "0", 0), ("ordered", "0", 1), ("atomic", "1", 1)])
def test_dq_route_from_the_environment(env, det, want):
    """BIGDL_ATTN_DQ and BIGDL_DETERMINISTIC as a fresh process reads them (the route query needs no GPU)."""
    code = "from bigdl_amd.ops import native; print('ROUTE', native.get().attn_dq_ordered())"
    e = dict(os.environ, BIGDL_DETERMINISTIC=det, PYTHONPATH=ROOT)
    e.pop("BIGDL_ATTN_DQ", None)
    if env:
        e["BIGDL_ATTN_DQ"] = env
    out = subprocess.run([sys.executable, "-c", code], env=e, cwd=ROOT, capture_output=True, text=True, check=True)
    assert f"ROUTE {want}" in out.stdout, out.stdout + out.stderr
