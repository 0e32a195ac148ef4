"""csrc/attn_decode.hip element by element: attn_decode against softmax(q k^T + bias) v in fp64 on the bf16-rounded
operands, kv_append and kv_reorder bit for bit.

Tolerance (the rule of test_attention_edges_gpu.py, the flash kernel's yardstick): per element
|kernel - exact| <= 3 E + 1e-6 max|exact|, E = max |reference with P rounded to bf16 - exact|, from the reference
alone. The bias is added the way the kernel and the fp32 math path add it, (s.float() + bias).double(): a -1e9 entry
absorbs the score, which matters only for rows whose every key carries -1e9 (the uniform average). The decode kernel
never rounds P, so its ratios sit far below 1; the largest seen on an MI355X are in
profiles/decode_native_errors.txt.

Lengths: 1, 2, 63, 64, 65, 130 and both sides of every keys-per-wave-pass (4, 8, 16) and keys-per-workgroup-pass
(16, 32, 64) of the kernel. Cache and bias positions >= len hold NaN. torch.matmul / softmax / cat / gather raise
while the native calls run.
"""
import pytest
import torch

from tests.beam_decode_cases import aten_guard

pytestmark = pytest.mark.gpu

NEG = -1e9
LENS = sorted({1, 2, 63, 64, 65, 130, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33})
N = 5
ROWS = [2, 0, 0, 1, 2]


def _reference(q, k, v, bias):
    """q [N, H, D], k / v [N, L, H, D] (already gathered through rows), bias [N, L] or None, all bf16-representable
    fp32 on the CPU. Returns exact [N, H * D] (fp64) and E."""
    q64, k64, v64 = q.double(), k.double().transpose(1, 2), v.double().transpose(1, 2)     # [N, H, L, D]
    s = torch.einsum("nhd,nhld->nhl", q64, k64)
    if bias is not None:
        s = (s.float() + bias.float().unsqueeze(1)).double()
    dead = torch.isinf(s).all(-1, keepdim=True)
    P = torch.softmax(torch.where(dead, torch.zeros_like(s), s), -1)
    P = torch.where(dead, torch.zeros_like(P), P)       # every key -inf: pinned as 0
    exact = torch.einsum("nhl,nhld->nhd", P, v64)
    rounded = torch.einsum("nhl,nhld->nhd", P.float().bfloat16().double(), v64)
    E = (rounded - exact).abs().max().item()
    return exact.reshape(q.shape[0], -1), E


def _bias(kind, R, L, Lmax):
    b = torch.zeros(R, Lmax)
    b[:, L - L // 4:L] = NEG                             # the last quarter of the keys
    b[0, :L] = NEG                                       # row 0: all but one key masked
    b[0, L // 2] = 0.0
    b[1, :L] = NEG if kind == "neg" else float("-inf")   # row 1: every key masked
    b[:, L:] = float("nan")
    return b


@pytest.mark.parametrize("D", [32, 64, 96, 128])
@pytest.mark.parametrize("mode", ["identity", "rows_neg", "rows_inf"])
def test_attn_decode_against_fp64(D, mode):
    from bigdl_amd.ops.attention import decode_attention

    torch.manual_seed(11 + D)
    worst = 0.0
    for heads in (1, 3):
        hidden = heads * D
        for L in LENS:
            Lmax = L + 7
            R = N if mode == "identity" else 3
            q = (torch.randn(N, hidden) * D ** -0.5)
            kc = torch.randn(R, Lmax, hidden).bfloat16()
            vc = torch.randn(R, Lmax, hidden).bfloat16()
            kc[:, L:] = float("nan")
            vc[:, L:] = float("nan")
            rows = None if mode == "identity" else torch.tensor(ROWS, dtype=torch.int32)
            bias = None if mode == "identity" else _bias("neg" if mode == "rows_neg" else "inf", R, L, Lmax)
            with aten_guard():
                o = decode_attention(q.cuda(), kc.cuda(), vc.cuda(), L, heads,
                                     None if rows is None else rows.cuda(), None if bias is None else bias.cuda())
                torch.cuda.synchronize()
            o = o.cpu()
            assert o.shape == (N, hidden) and o.dtype == torch.float32
            assert not torch.isnan(o).any(), (heads, L)          # nothing past len reaches the output
            ix = torch.arange(N) if rows is None else rows.long()
            qr = q.bfloat16().float().view(N, heads, D)          # the kernel rounds q on load
            kr = kc[ix, :L].float().view(N, L, heads, D)
            vr = vc[ix, :L].float().view(N, L, heads, D)
            exact, E = _reference(qr, kr, vr, None if bias is None else bias[ix, :L])
            err = (o.double() - exact).abs()
            bound = 3 * E + 1e-6 * exact.abs().max().item()
            ratio = err.max().item() / E if E > 0 else float(err.max().item() > 0)
            worst = max(worst, ratio)
            assert (err <= bound).all(), (heads, L, err.max().item(), E)
            if mode != "identity":
                only = L // 2                                    # all but one key masked: that key's value row
                for n in (1, 2):                                 # sequences 1 and 2 read cache row 0
                    if L > 1:
                        assert torch.equal(o[n], vc[0, only].float()), (heads, L)
                if mode == "rows_neg":                           # every key -1e9: the uniform average
                    mean = vc[1, :L].double().mean(0)
                    assert (o[3].double() - mean).abs().max().item() <= 1e-5 * max(1.0, mean.abs().max().item())
                else:                                            # every key -inf: zeros
                    assert (o[3] == 0).all()
    print(f"DECODE_RATIO attn_decode D={D} {mode} worst_err_over_E={worst:.4f}")


def test_attn_decode_clamps_rows_and_checks_arguments():
    from bigdl_amd.ops import native
    from bigdl_amd.ops.attention import decode_attention

    torch.manual_seed(3)
    heads, D, L, Lmax, R = 2, 32, 9, 12, 3
    q = torch.randn(N, heads * D, device="cuda")
    kc = torch.randn(R, Lmax, heads * D, device="cuda").bfloat16()
    vc = torch.randn(R, Lmax, heads * D, device="cuda").bfloat16()
    wild = torch.tensor([-1, 3, 100, 1, 0], dtype=torch.int32, device="cuda")
    tame = torch.tensor([0, 2, 2, 1, 0], dtype=torch.int32, device="cuda")
    assert torch.equal(decode_attention(q, kc, vc, L, heads, wild), decode_attention(q, kc, vc, L, heads, tame))
    C = native.get()
    o = torch.empty_like(q)
    for bad in (0, Lmax + 1):
        with pytest.raises(RuntimeError):
            C.attn_decode(q, kc, vc, bad, heads, tame, None, o)
    with pytest.raises(RuntimeError):
        C.attn_decode(q, kc.float(), vc.float(), L, heads, tame, None, o)            # dtype
    with pytest.raises(RuntimeError):
        C.attn_decode(q, kc.transpose(0, 1), vc.transpose(0, 1), L, heads, tame, None, o)   # contiguity
    with pytest.raises(RuntimeError):
        C.attn_decode(q, kc, vc, L, 4, tame, None, o)                                # D = 16
    with pytest.raises(RuntimeError):
        C.attn_decode(q, kc, vc, L, heads, None, None, o)                            # no rows but R != N


def test_other_head_dims_take_the_math_path(monkeypatch):
    """D = 48 is outside the kernel's set: the torch math of the same signature runs on the bf16 cache, with q
    rounded like the kernel rounds it (fp32 sums over 9 keys and 48 columns: 1e-5 of the largest value)."""
    from bigdl_amd.ops import attention as att

    torch.manual_seed(4)
    heads, D, L, Lmax, R = 2, 48, 9, 12, 3
    q = torch.randn(N, heads * D) * D ** -0.5
    kc, vc = torch.randn(R, Lmax, heads * D).bfloat16(), torch.randn(R, Lmax, heads * D).bfloat16()
    kc[:, L:] = float("nan")
    vc[:, L:] = float("nan")
    rows = torch.tensor(ROWS, dtype=torch.int32)
    bias = _bias("neg", R, L, Lmax)
    calls = []
    real = att.decode_attention_math
    monkeypatch.setattr(att, "decode_attention_math", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    o = att.decode_attention(q.cuda(), kc.cuda(), vc.cuda(), L, heads, rows.cuda(), bias.cuda()).cpu()
    assert calls == [1]
    ix = rows.long()
    exact, _ = _reference(q.bfloat16().float().view(N, heads, D), kc[ix, :L].float().view(N, L, heads, D),
                          vc[ix, :L].float().view(N, L, heads, D), bias[ix, :L])
    assert (o.double() - exact).abs().max().item() <= 1e-5 * exact.abs().max().item()


@pytest.mark.parametrize("hidden", [64, 72])
def test_kv_append_bitwise(hidden):
    from bigdl_amd.ops.attention import kv_append

    torch.manual_seed(5)
    Lmax = 6
    for pos in (0, 3, 5):
        k, v = torch.randn(N, hidden), torch.randn(N, hidden)
        poison = lambda: torch.full((N, Lmax, hidden), 0x7a7a, dtype=torch.int16).view(torch.bfloat16)  # noqa: E731
        kc, vc = poison().cuda(), poison().cuda()
        with aten_guard():
            kv_append(k.cuda(), v.cuda(), kc, vc, pos)
            torch.cuda.synchronize()
        wk, wv = poison(), poison()
        wk[:, pos], wv[:, pos] = k.bfloat16(), v.bfloat16()
        assert torch.equal(kc.cpu().view(torch.int16), wk.view(torch.int16))
        assert torch.equal(vc.cpu().view(torch.int16), wv.view(torch.int16))


@pytest.mark.parametrize("hidden", [64, 72])
@pytest.mark.parametrize("length", [1, 9])
def test_kv_reorder_bitwise(hidden, length):
    from bigdl_amd.ops import native
    from bigdl_amd.ops.attention import kv_reorder

    torch.manual_seed(6)
    layers, n, Lmax = 2, 6, 12
    src = torch.randn(layers, 2, n, Lmax, hidden).bfloat16()
    dst = torch.full((layers, 2, n, Lmax, hidden), 0x7a7a, dtype=torch.int16).view(torch.bfloat16)
    parent = torch.tensor([1, 1, 0, 5, 3, 3], dtype=torch.int32)
    want = dst.clone()
    want[:, :, :, :length] = src.index_select(2, parent.long())[:, :, :, :length]
    s, d = src.cuda(), dst.cuda()
    with aten_guard():
        kv_reorder(s, d, parent.cuda(), length)
        torch.cuda.synchronize()
    assert torch.equal(d.cpu().view(torch.int16), want.view(torch.int16))        # dst beyond len untouched
    assert torch.equal(s.cpu().view(torch.int16), src.view(torch.int16))
    with pytest.raises(RuntimeError):
        native.get().kv_reorder(s, s, parent.cuda(), length)                      # never in place
