"""Cases, data and fp64 references for the convolution kernels (csrc/conv_igemm.hip, conv_halo.hip, stem_fwd.hip,
wgrad_halo.hip, conv_epilogue.h), shared by tests/test_conv_edges_gpu.py (kernel vs reference, element by element)
and tests/test_conv_edges_cpu.py (the reference's own sanity and the sensitivity the GPU tests rely on). Everything
here runs on the CPU.

Two legs over one table of routes:

* exact: small integers (x, dy in [-4, 4], w in [-2, 2], bias in [-8, 8], addend in [-16, 16]; a BN applied on load has
  a scale in {0.5, 1, 2} and an integer shift). Every product and every partial sum is then a multiple of the
  quantum (1, or 0.5 behind such a BN: ``quantum``) below 2^24 quanta, i.e. exact in fp32 whatever the accumulation
  order, split-K or atomics, so the bf16 output is defined bit for bit: the fp64 result rounded to nearest even
  (csrc/common.h f2bf). ``exactness_bound`` is the largest magnitude any partial sum can reach. Part of the data is
  drawn coherently (``nt_inputs``) so that every case has outputs above 256, where bf16 really rounds.
* gauss: bf16-rounded Gaussian data, full mantissas; per element |got - ref| <= 2^-8 |ref| + 2 Kdim 2^-24 A with A
  the same operation over absolute values (``nt_bound``).

The fused reductions (BN statistics of the rounded output; the consumer BN's backward sums of the rounded gradient)
are referred to fp64 sums over the *expected* tensors. Their terms are exact in fp32 (a bf16 value squared has 16
significant bits; d * (x - mean) is a small integer times a bf16 integer), so the only error is the summation's:
equality where ``n * max|term|`` stays below 2^24 quanta, else 2 n 2^-24 sum|terms| per channel (the running-error
bound of n fp32 additions in any order, times 2 for the slot / atomic order).
"""
import functools
from dataclasses import dataclass

import torch
import torch.nn.functional as F

U24 = 2.0 ** -24
BF16_ULP = 2.0 ** -8
XMAX, WMAX, BMAX, AMAX = 4, 2, 8, 16

# every conv switch a case may touch, at its default (csrc/conv_igemm.hip ConvSwitches, conv_halo.hip, stem_fwd.hip,
# wgrad_halo.hip); a case's own settings override these and the harness puts these back afterwards
DEFAULT_SWITCHES = {
    "set_conv_impl": 1, "set_conv_g4": 3, "set_conv_shortk": 0, "set_conv_p8": 1, "set_conv_w8": 0, "set_conv_sk": 0,
    "set_conv_s1": 2, "set_conv_halo": 1, "set_dgrad_s2": 1, "set_stem_fwd": 1, "set_stem_wgrad": 1,
    "set_wgrad_p8": 1, "set_wgrad_g3": 0, "set_wgrad_halo": 1, "set_wgrad_tr_asm": 1,
}

# conv_nt_plan_info operand flags
BIAS, STATS, ADDEND, RELU, BNRED, BNRED_Z, PRE, OUT32 = 1, 2, 4, 8, 16, 32, 64, 128


def out_size(inp, k, s, p):
    return (inp + 2 * p - k) // s + 1


@dataclass(frozen=True)
class NT:
    """A forward / data-gradient row: conv (N, C, H, W) -> (N, K, OH, OW), R x R, stride st, pad pd, under the
    switches ``sw``. ``fwd`` / ``dgrad``: the (kernel, BM, BN, stages) conv_nt_plan_info must report for the forward
    GEMM / for every stride phase of the data gradient (None: that direction is not run; "s2": the one-pass stride-2
    halo data gradient, which has no plan entry and reports by its return value). ``masks``: consumer-BN ReLU masks
    the data gradient runs under ("aff" from x * scale + shift, "z" a bf16 tensor, "zm" sign-mask bytes).
    ``pre``: also a forward with a BN applied on load; ``out32``: also an fp32 accumulate call; ``sub``: also a data
    gradient with a 2 x 2-subsampled addend; ``pair``: the 7 x 8 / stride-2 pixel-pair stem over 4-channel pairs;
    ``slice`` = c0 > 0: also a forward written in place into channels [c0, c0 + K) of a (c0 + K + c0)-channel buffer
    (a concat slice: row stride above Ncol), whose other channels must stay untouched; ``wd``: the image width where it is not the height H."""
    name: str
    geom: tuple
    sw: tuple = ()
    fwd: tuple = None
    dgrad: object = None
    masks: tuple = ("aff",)
    pre: bool = False
    out32: bool = False
    sub: bool = False
    pair: bool = False
    slice: int = 0
    wd: int = 0

    def __str__(self):
        return self.name

    @property
    def dims(self):
        N, C, H, K, R, st, pd = self.geom
        return N, C, H, K, R, st, pd, out_size(H, R, st, pd)

    @property
    def W(self):
        return self.wd or self.geom[2]

    @property
    def OW(self):
        return out_size(self.W, *self.geom[4:])

    @property
    def kdim_fwd(self):
        return self.geom[4] ** 2 * self.geom[1]

    @property
    def kdim_dgrad(self):
        return self.geom[4] ** 2 * self.geom[3]


def _sw(**kw):
    return tuple(sorted(("set_" + k, v) for k, v in kw.items()))


def _n(tag, geom, sw=(), **kw):
    wide = f"-w{kw['wd']}" if kw.get("wd") else ""
    return NT(f"{tag}-" + "x".join(map(str, geom)) + wide, geom, sw, **kw)


G3, G4S, G7 = ("g4", 128, 64, 3), ("g4", 128, 64, 4), ("g4", 256, 128, 3)
G3W, G4W = ("g4", 128, 128, 3), ("g4", 128, 128, 4)
S1, HALO = ("s1", 0, 0, 0), ("halo", 0, 0, 0)
P8 = ("p8", 256, 256, 0)
P8S = ("p8_split", 256, 256, 0)
P8K = ("p8_sk", 256, 256, 0)
W8, W8S = ("w8", 256, 256, 0), ("w8_split", 256, 256, 0)


def _g4_rows():
    """The multi-stage kernel in its four tile / stage forms (g4 3 / 4 / 7, shortk), s1 / halo / p8 off so that the
    1x1 and 3x3 shapes stay on it. M tiles of 128 (256 under g4 7), N tiles of 64 / 128, K steps of 32."""
    rows = []
    shapes = [(2, 64, 12, 64, 3, 1, 1),      # M 288 = 2 tiles + 32, one 64-column tile
              (4, 64, 14, 64, 1, 2, 0),      # stride 2: M 196 (tile + 68); dgrad writes a strided placement
              (2, 80, 9, 200, 1, 1, 0),      # Cs 80 (not a multiple of 32: per-lane taps), Ncol 200 = 128 + 72
              (3, 40, 11, 64, 3, 2, 1),      # Cs 40, stride 2 + pad 1: four dgrad phases with 1 / 2 / 2 / 4 taps
              (4, 96, 14, 128, 3, 1, 1)]     # three 32-channel K steps per tap, M 784 = 6 tiles + 16
    for g4 in (3, 4, 7):
        for geom in shapes:
            N, C, H, K, R, st, pd = geom
            sw = _sw(conv_g4=g4, conv_s1=0, conv_halo=0, conv_p8=0, dgrad_s2=0)

            def form(ncol):
                if g4 == 7 and ncol > 64:
                    return G7
                wide = ncol > 64
                return (G4W if wide else G4S) if g4 == 4 else (G3W if wide else G3)

            rows.append(_n(f"g4_{g4}", geom, sw, fwd=form(K), dgrad=form(C), masks=("aff", "z", "zm"),
                           out32=(g4 == 3 and geom == shapes[0]), slice=8 * (geom in (shapes[0], shapes[2]))))
    # shortk: Kdim <= 64 and Ncol <= 64, both directions
    rows.append(_n("g4_shortk", (4, 64, 14, 64, 1, 2, 0), _sw(conv_shortk=1, conv_s1=0, conv_halo=0, conv_p8=0),
                   fwd=("g4", 128, 64, 2), dgrad=("g4", 128, 64, 2), masks=("aff", "z", "zm")))
    return rows


NT_CASES = (
    # register-staged kernel (impl 0): Cs 40 (slow K), Ncol 72 / 24, and an output whose rows are not 16-byte
    # multiples (K 20: the fallback epilogue; its data gradient would have Cs 20, which no kernel takes)
    [_n("reg", (1, 40, 9, 72, 3, 1, 1), _sw(conv_impl=0), fwd=("reg", 128, 128, 1), dgrad=("reg", 128, 64, 1),
        masks=("aff", "z", "zm"), slice=8),
     _n("reg", (1, 40, 9, 24, 3, 1, 1), _sw(conv_impl=0), fwd=("reg", 128, 64, 1), dgrad=("reg", 128, 64, 1),
        masks=("aff", "z", "zm")),
     _n("reg", (2, 64, 9, 72, 1, 1, 0), _sw(conv_impl=0), fwd=("reg", 128, 128, 1), dgrad=("reg", 128, 64, 1)),
     _n("reg_unaligned", (3, 40, 7, 20, 3, 1, 1), _sw(conv_impl=0), fwd=("reg", 128, 64, 1), slice=4)]
    # LDS-DMA kernels (impl 1, g4 0; s1 / halo off): two-stage, single-stage (Kdim 64) and slow-K (Cs 40)
    + [_n("glds", (2, 64, 9, 136, 3, 1, 1), _sw(conv_g4=0, conv_s1=0, conv_halo=0), fwd=("glds", 128, 128, 2),
          dgrad=("glds_slowk", 128, 64, 2), masks=("aff", "z", "zm"), slice=8),
       _n("glds", (2, 128, 9, 64, 3, 1, 1), _sw(conv_g4=0, conv_s1=0, conv_halo=0), fwd=("glds", 128, 64, 2),
          dgrad=("glds", 128, 128, 2), masks=("aff", "z", "zm")),
       _n("glds_onestage", (3, 64, 13, 72, 1, 2, 0), _sw(conv_g4=0, conv_s1=0, conv_halo=0),
          fwd=("glds_onestage", 128, 128, 1), dgrad=("glds_slowk", 128, 64, 2), masks=("aff", "z", "zm")),
       _n("glds_slowk", (2, 40, 9, 136, 3, 1, 1), _sw(conv_g4=0, conv_s1=0, conv_halo=0),
          fwd=("glds_slowk", 128, 128, 2), dgrad=("glds_slowk", 128, 64, 2), masks=("aff", "z", "zm"))]
    + _g4_rows()
    # images wider or narrower than high (a row / column mix-up passes every square case), on the kernels that take them
    + [_n("reg", (2, 40, 9, 72, 3, 1, 1), _sw(conv_impl=0), fwd=("reg", 128, 128, 1), dgrad=("reg", 128, 64, 1), wd=12),
       _n("glds", (2, 64, 11, 136, 3, 1, 1), _sw(conv_g4=0, conv_s1=0, conv_halo=0), fwd=("glds", 128, 128, 2),
          dgrad=("glds_slowk", 128, 64, 2), wd=7),
       _n("g4_3", (3, 32, 9, 48, 3, 2, 1), _sw(conv_g4=3, conv_s1=0, conv_halo=0, conv_p8=0, dgrad_s2=0), fwd=G3,
          dgrad=G3, masks=("aff", "zm"), wd=11),
       _n("g4_7", (4, 96, 14, 128, 3, 1, 1), _sw(conv_g4=7, conv_s1=0, conv_halo=0, conv_p8=0), fwd=G7, dgrad=G7, wd=9),
       _n("s1", (3, 64, 7, 64, 1, 1, 0), fwd=S1, dgrad=S1, masks=("aff", "zm"), sub=True, wd=12),
       _n("p8_split", (3, 64, 10, 512, 3, 1, 1), _sw(conv_p8=2), fwd=P8S, dgrad=P8S, wd=7)]
    # deep-pipelined 256-pixel kernel (impl 2): 30 x 9 tiles with an M tail of 18 rows and an Ncol tail of 8; its
    # 64-column form at the smallest M with 256 tiles (65 348 rows: tail 68)
    + [_n("p3", (2, 64, 61, 1032, 1, 1, 0), _sw(conv_impl=2), fwd=("p3", 256, 128, 0), slice=8),
       _n("p3_n64", (17, 64, 62, 64, 1, 1, 0), _sw(conv_impl=2), fwd=("p3", 256, 64, 0), dgrad=("p3", 256, 64, 0),
          masks=("aff", "z", "zm"))]
    # persistent kernel (impl 3): 59 x 10 = 590 tiles on 512 workgroups, so the tile loop runs twice
    + [_n("pers", (2, 64, 61, 1160, 1, 1, 0), _sw(conv_impl=3), fwd=("pers", 128, 128, 2), slice=8),
       # its data gradient: 262 x 2 = 524 tiles (the forward of this shape has 262 and stays on the 2-stage kernel)
       _n("pers_dgrad", (9, 256, 61, 128, 1, 1, 0), _sw(conv_impl=3), dgrad=("pers", 128, 128, 2), masks=("aff", "z", "zm"))]
    # streaming 1x1 kernel: Kdim 64 / 128 / 256, one to four channel groups, M tails
    + [_n("s1", (1, 64, 5, 64, 1, 1, 0), fwd=S1, dgrad=S1, masks=("aff", "zm")),
       _n("s1", (5, 64, 13, 64, 1, 1, 0), fwd=S1, dgrad=S1, masks=("aff", "zm"), sub=True),
       _n("s1", (3, 128, 11, 192, 1, 1, 0), fwd=S1, pre=True, slice=8),
       _n("s1", (3, 128, 11, 128, 1, 1, 0), fwd=S1, dgrad=S1, masks=("aff", "zm")),
       _n("s1", (1, 256, 9, 128, 1, 1, 0), fwd=S1, pre=True),
       _n("s1", (2, 256, 9, 256, 1, 1, 0), fwd=S1, dgrad=S1, masks=("zm",))]
    # halo-tile 3x3 kernel: every width it takes at batch 1 and 32 channels; a second tile holding one of three
    # image slots; three 32-channel chunks; BN on load; the data gradient wherever the input channels allow
    + [_n("halo", (1, 32, 56, 64, 3, 1, 1), fwd=HALO, pre=True),
       _n("halo", (1, 64, 56, 64, 3, 1, 1), fwd=HALO, dgrad=HALO, masks=("aff", "zm")),
       _n("halo", (1, 32, 28, 128, 3, 1, 1), fwd=HALO, slice=8),
       _n("halo", (1, 32, 14, 128, 3, 1, 1), fwd=HALO),
       _n("halo", (1, 32, 7, 128, 3, 1, 1), fwd=HALO),
       _n("halo", (4, 32, 7, 128, 3, 1, 1), fwd=HALO),
       _n("halo", (4, 128, 7, 128, 3, 1, 1), fwd=HALO, dgrad=HALO, masks=("aff", "z", "zm")),
       _n("halo", (3, 96, 14, 128, 3, 1, 1), fwd=HALO, pre=True),
       _n("halo", (2, 128, 28, 128, 3, 1, 1), fwd=HALO, dgrad=HALO, masks=("zm",)),
       _n("halo", (2, 128, 14, 128, 3, 1, 1), fwd=HALO, dgrad=HALO, masks=("aff", "zm"))]
    # one-pass stride-2 data gradient from halo tiles of dy: its three widths (dy 7, 14 and 28), the smallest
    # geometries it takes
    + [_n("halo_s2", (1, 32, 14, 32, 3, 2, 1), dgrad="s2", masks=("aff", "zm")),
       _n("halo_s2", (1, 32, 56, 32, 3, 2, 1), dgrad="s2", masks=("aff", "zm")),
       _n("halo_s2", (3, 72, 28, 64, 3, 2, 1), dgrad="s2", masks=("aff", "zm"))]
    # 256 x 256 phase-interleaved kernel (p8 2): one pass, split-K, the one-tap K tail, stream-K
    + [_n("p8", (2, 192, 9, 256, 1, 1, 0), _sw(conv_p8=2), fwd=P8, slice=8),
       _n("p8_split", (3, 64, 10, 512, 3, 1, 1), _sw(conv_p8=2), fwd=P8S, dgrad=P8S, masks=("aff", "z", "zm"), slice=8),
       _n("p8_ktail", (8, 200, 14, 256, 1, 1, 0), _sw(conv_p8=2), fwd=P8, dgrad=P8, masks=("aff", "z", "zm")),
       _n("p8_ktail_dgrad", (4, 256, 9, 520, 1, 1, 0), _sw(conv_p8=2, conv_s1=0), fwd=P8, dgrad=P8S, masks=("aff", "z", "zm")),
       _n("p8_sk", (8, 512, 32, 1024, 1, 1, 0), _sw(conv_sk=2), fwd=P8K, dgrad=P8K, masks=("aff", "z", "zm"))]
    # 256 x 256 8-wave kernel (w8 1)
    + [_n("w8", (2, 192, 9, 256, 1, 1, 0), _sw(conv_w8=1), fwd=W8, slice=8),
       _n("w8", (2, 256, 9, 256, 1, 1, 0), _sw(conv_w8=1, conv_s1=0), fwd=W8, dgrad=W8, masks=("aff", "z", "zm")),
       _n("w8_split", (4, 512, 7, 2048, 1, 1, 0), _sw(conv_w8=1), fwd=W8S, dgrad=W8S, masks=("aff", "z", "zm"))]
    # 7x7 / stride-2 image stem over pixel pairs: 2 images x 8 output rows = 4 row tiles of the dedicated kernel
    + [NT("stem-2x21x115-8x112", (2, 8, 0, 64, 7, 2, 0), (), fwd=("stem", 0, 0, 0), pair=True)]
)
NT_BY_NAME = {c.name: c for c in NT_CASES}
assert len(NT_BY_NAME) == len(NT_CASES)

STEM_OH, STEM_OW, STEM_HP, STEM_WQ, STEM_S2 = 8, 112, 21, 115, 4


@dataclass(frozen=True)
class WG:
    """A weight-gradient row: the kernel conv_wgrad_ladder must pick (``kernel``) and its pixel split as
    conv_wgrad_plan_info reports it, with the bias gradient. ``wd``: the image width where it is not the height."""
    name: str
    geom: tuple
    sw: tuple
    kernel: str
    splits: int
    pair: bool = False
    wd: int = 0

    def __str__(self):
        return self.name

    @property
    def dims(self):
        N, C, H, K, R, st, pd = self.geom
        return N, C, H, K, R, st, pd, out_size(H, R, st, pd)

    @property
    def W(self):
        return self.wd or self.geom[2]

    @property
    def OW(self):
        return out_size(self.W, *self.geom[4:])


def _w(kernel, geom, splits, wd=0, **sw):
    return WG(f"{kernel}-" + "x".join(map(str, geom)) + (f"-w{wd}" if wd else ""), geom, _sw(**sw), kernel, splits,
              wd=wd)


WG_CASES = [
    # halo-tile 3x3 kernel with one split (adds into dW directly) and with many (workspace + reduce)
    _w("halo", (1, 64, 7, 64, 3, 1, 1), 1),
    _w("halo", (5, 64, 14, 192, 3, 1, 1), 35),
    # 256 x 256 kernel (wgrad_p8 2): GEMM-shaped (reads dy and x in place) and general, Ncol / Kdim tails of 8 + 64
    _w("p8_direct", (6, 264, 14, 320, 1, 1, 0), 2, wgrad_p8=2),
    _w("p8", (3, 72, 10, 264, 3, 2, 1), 1, wgrad_p8=2),
    _w("p8", (7, 72, 13, 264, 3, 1, 1), 2, wgrad_p8=2),          # M 1183: two splits of 640 and 543 pixels
    # 128 x 128 LDS-DMA kernels, 2-stage and 3-stage, through the workspace (M 2704 is not a multiple of the split's
    # pixel step) and through atomics (one split); Ncol 136 and Kdim 200 leave tails of 8
    _w("glds_ws", (4, 200, 26, 136, 1, 1, 0), 6),
    _w("g3_ws", (4, 200, 26, 136, 1, 1, 0), 6, wgrad_g3=1),
    _w("glds_ws", (6, 128, 28, 136, 3, 2, 1), 3),
    _w("glds_atomic", (2, 72, 9, 136, 3, 1, 1), 1),
    _w("g3_atomic", (2, 72, 9, 136, 3, 1, 1), 1, wgrad_g3=1),
    # register-staged atomic kernel: the default for <= 64 output channels over a deep reduction, and under impl 0
    _w("reg", (8, 40, 30, 48, 3, 1, 1), 0),
    _w("reg", (2, 72, 9, 136, 3, 1, 1), 0, conv_impl=0),
    # images wider than high
    _w("glds_ws", (4, 200, 20, 136, 1, 1, 0), 6, wd=34),
    _w("reg", (8, 40, 24, 48, 3, 1, 1), 0, wd=37),
    _w("p8", (7, 72, 11, 264, 3, 2, 1), 1, wd=16, wgrad_p8=2),
    # pair-view stem kernel
    WG("stem-2x21x115-8x112", (2, 8, 0, 64, 7, 2, 0), (), "stem", -1, pair=True),
]
WG_BY_NAME = {c.name: c for c in WG_CASES}
assert len(WG_BY_NAME) == len(WG_CASES)


# ------------------------------------------------------------------------------------------------------------------
# data
# ------------------------------------------------------------------------------------------------------------------
def _gen(case, salt):
    table = NT_CASES if isinstance(case, NT) else WG_CASES
    g = torch.Generator()
    g.manual_seed((table.index(case) * 2 + isinstance(case, WG)) * 64 + salt)
    return g


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _signs(g, n):
    return torch.randint(0, 2, (n,), generator=g).double() * 2 - 1


def _hot(g, base, signs, top):
    """``base`` with a random quarter of its pixels replaced by signs * (top - 1 or top)."""
    N, C, H, W = base.shape
    hot = torch.rand(N, 1, H, W, generator=g) < 0.25
    return torch.where(hot, signs * _ints(g, top - 1, top, N, C, H, W), base)


def _r16(t):
    """Round to bf16 (nearest even) and back: fp64 values that bf16 holds."""
    return t.float().bfloat16().double()


def _x_shape(case):
    N, C, H, K, R, st, pd, OH = case.dims
    return (N, 4, STEM_HP, 2 * STEM_WQ) if case.pair else (N, C, H, case.W)


def _y_shape(case):
    N, C, H, K, R, st, pd, OH = case.dims
    return (N, K, STEM_OH, STEM_OW) if case.pair else (N, K, OH, case.OW)


def _w_shape(case):
    N, C, H, K, R, st, pd, OH = case.dims
    return (K, 4, 7, 8) if case.pair else (K, C, R, R)


@functools.lru_cache(maxsize=2)
def nt_inputs(case, leg):
    """fp64 CPU tensors, NCHW: x, w, bias, dy, addend (dx-shaped), sub (2 x 2-subsampled addend), the consumer BN's
    bx / bz / mean / aff, the on-load BN's pre (scale | shift) and out0 (the fp32 accumulate call's starting
    output). Every bf16 operand holds bf16 values in both legs."""
    g = _gen(case, 1 if leg == "int" else 2)
    xs, ys, ws = _x_shape(case), _y_shape(case), _w_shape(case)
    C, K = xs[1], ys[1]
    d = {}
    if leg == "int":
        # Uniform draws alone would keep |y| near sqrt(Kdim) * 3.7: no output of a 64-deep reduction would pass 256,
        # where bf16 starts to round integers. So a quarter of the pixels and of the weight columns and an eighth of the weight rows
        # are "hot": their signs follow one per-channel pattern and their magnitudes sit at the top of the range, so
        # hot pixel x hot row sums coherently (about 7 per term), inside the same value ranges.
        sc, tk = _signs(g, C), _signs(g, K)
        d["x"] = _hot(g, _ints(g, -XMAX, XMAX, *xs), sc.view(1, C, 1, 1), XMAX)
        d["dy"] = _hot(g, _ints(g, -XMAX, XMAX, *ys), tk.view(1, K, 1, 1), XMAX)
        w = _ints(g, -WMAX, WMAX, *ws)
        mag = WMAX - (torch.rand(*ws, generator=g) < 0.25).double()        # mostly 2; some 1, so that sums are odd too
        w[:, 1::4] = (tk.view(K, 1, 1, 1) * mag)[:, 1::4]          # hot columns: coherent with hot dy pixels
        w[1::8] = (sc.view(1, C, 1, 1) * mag)[1::8]                # hot rows: coherent with hot x pixels
        w[7::8] = mag[7::8]                                        # positive rows: coherent behind a BN + ReLU on load
        d["w"] = w
        d["bias"] = _ints(g, -BMAX, BMAX, K)
        d["addend"] = _ints(g, -AMAX, AMAX, *xs)
        d["bx"] = _ints(g, -XMAX, XMAX, *xs)
        d["bz"] = torch.relu(_ints(g, -3, 3, *xs))
        d["mean"] = _ints(g, -2, 2, C)
        d["out0"] = _ints(g, -BMAX, BMAX, *ys)
    else:
        kdim = ws[1] * ws[2] * ws[3]
        d["x"] = _r16(torch.randn(*xs, generator=g))
        d["w"] = _r16(torch.randn(*ws, generator=g) * kdim ** -0.5)
        d["bias"] = torch.randn(K, generator=g).float().double()
        d["dy"] = _r16(torch.randn(*ys, generator=g))
        d["addend"] = _r16(torch.randn(*xs, generator=g))
        d["bx"] = _r16(torch.randn(*xs, generator=g))
        d["bz"] = _r16(torch.relu(torch.randn(*xs, generator=g)))
        d["mean"] = torch.randn(C, generator=g).float().double()
        d["out0"] = torch.randn(*ys, generator=g).float().double()
    d["sub"] = d["addend"][:, :, ::2, ::2].contiguous()
    # affine of the consumer BN's ReLU mask and the BN applied on load: power-of-two scales and integer shifts, so
    # x * scale + shift is one fp32 rounding with or without an FMA
    pick = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)
    d["aff"] = torch.cat([pick[torch.randint(0, 3, (C,), generator=g)], _ints(g, -2, 2, C)])
    d["pre"] = torch.cat([pick[torch.randint(0, 3, (C,), generator=g)], _ints(g, -2, 2, C)])
    return d


def pre_apply(case, leg):
    """What the kernel multiplies when a BN + ReLU is applied on load: bf16(relu(fp32(x * scale + shift)))."""
    d = nt_inputs(case, leg)
    C = d["x"].shape[1]
    sc, sh = d["pre"][:C].view(1, C, 1, 1), d["pre"][C:].view(1, C, 1, 1)
    return _r16(torch.relu((d["x"] * sc + sh).float().double()))


def quantum(case, op):
    """The unit every value of the exact leg is a multiple of: 0.5 behind a BN on load with scale 0.5, else 1."""
    return 0.5 if op.startswith("pre") else 1.0


# ------------------------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------------------------
def _conv(case, x, w):
    N, C, H, K, R, st, pd, OH = case.dims
    if case.pair:
        return F.conv2d(x, w, stride=2)
    return F.conv2d(x, w, stride=st, padding=pd)


def _conv_t(case, dy, w):
    N, C, H, K, R, st, pd, OH = case.dims
    return torch.nn.grad.conv2d_input((N, C, H, case.W), w, dy, stride=st, padding=pd)


FWD_OPS = ("bias_stats", "bias_relu")


def fwd_ops(case):
    ops = list(FWD_OPS) if case.fwd else []
    if case.pre:
        ops.append("pre_bias_stats")
    if case.out32:
        ops.append("out32_acc")
    if case.slice:
        ops.append("slice_bias_stats")
    return ops


def covered(case):
    """Does a stride phase of the data gradient reach every input pixel? (Row a of a stride period is reached when
    some tap r has (a + pad - r) % stride == 0.) Where not, conv2d_dgrad fills the other pixels from the addend in a
    pass of its own and the call carries no consumer-BN reduction."""
    N, C, H, K, R, st, pd, OH = case.dims
    return all(any((a + pd - r) % st == 0 for r in range(R)) for a in range(st))


def dgrad_ops(case):
    """"add_bnred_<mask>": addend + consumer-BN reduction; "bnred_<mask>": the reduction alone; "add": the addend
    alone (once: no mask is involved), on the geometries that are not ``covered``."""
    if not case.dgrad:
        return []
    ops = [] if covered(case) or case.dgrad == "s2" else ["add"]
    for m in case.masks:
        if case.dgrad != "s2" and covered(case):            # (the one-pass stride-2 kernel takes no addend)
            ops.append(f"add_bnred_{m}")
        ops.append(f"bnred_{m}")
    if case.sub:
        ops.append("sub_bnred_aff")
    return ops


def op_flags(op):
    """conv_nt_plan_info flags of an op."""
    if op in ("bias_stats", "slice_bias_stats"):
        return BIAS | STATS
    if op == "bias_relu":
        return BIAS | RELU
    if op == "pre_bias_stats":
        return BIAS | STATS | PRE
    if op == "out32_acc":
        return OUT32
    if op == "add":
        return ADDEND
    kind, mask = op.rsplit("_", 1)
    f = BNRED_Z if mask == "z" else BNRED
    return f | (ADDEND if kind != "bnred" else 0)


@functools.lru_cache(maxsize=2)
def _fwd_core(case, leg, pre):
    x, w = (pre_apply(case, leg) if pre else nt_inputs(case, leg)["x"]), nt_inputs(case, leg)["w"]
    return _conv(case, x, w), _conv(case, x.abs(), w.abs())


@functools.lru_cache(maxsize=2)
def _dgrad_core(case, leg):
    d = nt_inputs(case, leg)
    return _conv_t(case, d["dy"], d["w"]), _conv_t(case, d["dy"].abs(), d["w"].abs())


def nt_exact(case, leg, op, fault=None):
    """fp64 result of ``op`` before the output rounding. Returns (y, A): the value and the same operation over
    absolute values (the Gaussian leg's error scale). ``fault`` (CPU sensitivity checks): see FAULTS."""
    d = nt_inputs(case, leg)
    x, w = d["x"], d["w"]
    K = w.shape[0]
    if op == "slice_bias_stats":
        op = "bias_stats"
    if op in FWD_OPS + ("pre_bias_stats", "out32_acc"):
        y, A = _fwd_core(case, leg, op == "pre_bias_stats")
        if fault:
            y = _faulty_conv(case, x, w, fault)
        if op == "out32_acc":
            return y + d["out0"], A + d["out0"].abs()
        b = d["bias"].view(1, K, 1, 1)
        y, A = y + b, A + b.abs()
        if op == "bias_relu":
            y = torch.relu(y)
        return y, A
    assert fault is None
    dx, A = _dgrad_core(case, leg)
    if op.startswith("add"):
        dx, A = dx + d["addend"], A + d["addend"].abs()
    elif op.startswith("sub_"):
        full = torch.zeros_like(dx)
        full[:, :, ::2, ::2] = d["sub"]
        dx, A = dx + full, A + full.abs()
    return dx, A


def round_bf16(y):
    """The kernels' output rounding: fp64 -> fp32 -> bf16, nearest even (torch's cast; csrc/common.h f2bf)."""
    return y.float().bfloat16()


def trunc_bf16(y):
    """The wrong rounding: the fp32 value's low 16 bits cut off."""
    bits = y.float().contiguous().view(torch.int32) & -65536
    return bits.view(torch.float32).bfloat16()


def nt_bound(case, op, y, A):
    """Gaussian leg, per element: 2^-8 |ref| + the running-error bound of Kdim fp32 additions in any order, times
    2, on the absolute-value result. 2^-8 |ref| is a whole bf16 ulp (twice what nearest-even rounding can lose) at
    the top of a binade but only half an ulp just above a power of two: there correct rounding alone comes
    arbitrarily close to the first term, which is why observed ratios sit just under 1, and truncation (up to a
    whole ulp) exceeds it."""
    kdim = case.kdim_dgrad if op.split("_")[0] in ("add", "sub", "bnred") else case.kdim_fwd
    if case.pair:
        kdim = 224
    return BF16_ULP * y.abs() + 2 * kdim * U24 * A


def exactness_bound(case):
    """Largest magnitude a partial sum of the exact leg can reach, in quanta: Kdim max|x| max|w| + |bias| + |addend|
    over both directions (a BN on load scales x by at most 2 and shifts it by at most 2; its quantum is 0.5)."""
    kd = 224 if case.pair else max(case.kdim_fwd, case.kdim_dgrad if case.dgrad else 0)
    xmax = (2 * XMAX + 2) / 0.5 if case.pre else XMAX
    return kd * xmax * WMAX + BMAX + AMAX


def relu_mask(case, leg, mask):
    d = nt_inputs(case, leg)
    C = d["bx"].shape[1]
    if mask == "aff":
        return ((d["bx"] * d["aff"][:C].view(1, C, 1, 1) + d["aff"][C:].view(1, C, 1, 1)).float() > 0).double()
    return (d["bz"] > 0).double()


def reduction_ref(case, leg, op, out16):
    """The fused reduction of ``op`` over the expected rounded output ``out16`` (bf16): fp64 per-channel (s1, s2),
    and per channel whether equality is provable (n max|term| below 2^24 quanta) and the bound otherwise."""
    o = out16.double()
    n = o.numel() // o.shape[1]
    if op in ("bias_stats", "pre_bias_stats", "slice_bias_stats"):
        t1, t2 = o, o * o
        q1, q2 = quantum(case, op), quantum(case, op) ** 2
    else:
        d = nt_inputs(case, leg)
        m = relu_mask(case, leg, op.rsplit("_", 1)[1])
        t1 = o * m
        t2 = t1 * (d["bx"] - d["mean"].view(1, -1, 1, 1))
        q1 = q2 = 1.0
    res = []
    for t, q in ((t1, q1), (t2, q2)):
        s = t.sum(dim=(0, 2, 3))
        exact = n * t.abs().amax(dim=(0, 2, 3)) / q < 2.0 ** 24
        bound = 2 * n * U24 * t.abs().sum(dim=(0, 2, 3))
        res.append((s, exact, bound))
    return res


# ------------------------------------------------------------------------------------------------------------------
# injected faults (forward GEMM): what a kernel with a tile, tail or rounding bug would compute
# ------------------------------------------------------------------------------------------------------------------
FAULTS = ("drop_last_row", "drop_k_granule", "wrap_border_tap", "shift_columns")


def fault_applies(case, fault):
    N, C, H, K, R, st, pd, OH = case.dims
    if case.pair or not case.fwd:
        return False
    if fault == "wrap_border_tap":
        return pd > 0
    if fault == "shift_columns":
        return K >= 16
    return True


def _faulty_conv(case, x, w, fault):
    N, C, H, K, R, st, pd, OH = case.dims
    if fault == "drop_last_row":                # the last output pixel (last row of the last M tile) never written
        y = _conv(case, x, w).clone()
        y[N - 1, :, OH - 1, case.OW - 1] = 0
        return y
    if fault == "drop_k_granule":               # the reduction stops 8 channels short: last tap's last granule
        w2 = w.clone()
        w2[:, C - 8:, R - 1, R - 1] = 0
        return _conv(case, x, w2)
    if fault == "wrap_border_tap":
        # the tap one column left of the image reads the previous pixel of the flat NHWC tensor (the last column of
        # the row above, or of the previous image) instead of zero
        xp = F.pad(x, (pd, pd, pd, pd))
        W = case.W
        flat = x.permute(0, 2, 3, 1).reshape(N * H * W, C)
        prev = torch.cat([torch.zeros(1, C, dtype=x.dtype), flat[:-1]]).view(N, H, W, C)[:, :, 0, :]   # [N][H][C]
        xp[:, :, pd:pd + H, pd - 1] = prev.permute(0, 2, 1)
        return F.conv2d(xp, w, stride=st)
    if fault == "shift_columns":                # an output tile's 8-channel granules land one granule over
        return torch.roll(_conv(case, x, w), 8, dims=1)
    raise ValueError(fault)


def fault_rows(case, fault):
    """[N, OH, OW] bool: the output pixels the fault reaches, found by running it on all-ones data."""
    N, C, H, K, R, st, pd, OH = case.dims
    if fault == "shift_columns":
        return torch.ones(N, OH, case.OW, dtype=torch.bool)
    x, w = torch.ones(*_x_shape(case), dtype=torch.float64), torch.ones(*_w_shape(case), dtype=torch.float64)
    return ((_faulty_conv(case, x, w, fault) - _conv(case, x, w)) != 0).any(dim=1)


# ------------------------------------------------------------------------------------------------------------------
# weight gradient
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def wg_inputs(case, leg):
    """fp64 CPU tensors: x, dy (bf16 values), dw0 (K, C, R, S) and db0: the gradients the kernels add into."""
    g = _gen(case, 1 if leg == "int" else 2)
    xs, ys, ws = _x_shape(case), _y_shape(case), _w_shape(case)
    if leg == "int":
        return {"x": _ints(g, -XMAX, XMAX, *xs), "dy": _ints(g, -XMAX, XMAX, *ys),
                "dw0": _ints(g, -BMAX, BMAX, *ws), "db0": _ints(g, -BMAX, BMAX, ws[0])}
    return {"x": _r16(torch.randn(*xs, generator=g)), "dy": _r16(torch.randn(*ys, generator=g)),
            "dw0": torch.randn(*ws, generator=g).float().double(), "db0": torch.randn(ws[0], generator=g).float().double()}


@functools.lru_cache(maxsize=2)
def wg_reference(case, leg):
    """fp64 (dw, db, Aw, Ab): dw0 + the weight gradient, db0 + the column sums of dy, and the same over absolute
    values."""
    d = wg_inputs(case, leg)
    N, C, H, K, R, st, pd, OH = case.dims
    kw = dict(stride=2) if case.pair else dict(stride=st, padding=pd)

    def wgrad(x, dy):
        return torch.nn.grad.conv2d_weight(x, _w_shape(case), dy, **kw)

    dw = d["dw0"] + wgrad(d["x"], d["dy"])
    Aw = d["dw0"].abs() + wgrad(d["x"].abs(), d["dy"].abs())
    db = d["db0"] + d["dy"].sum(dim=(0, 2, 3))
    Ab = d["db0"].abs() + d["dy"].abs().sum(dim=(0, 2, 3))
    return dw, db, Aw, Ab


def wg_rows(case):
    """M: the pixels a weight gradient sums over."""
    ys = _y_shape(case)
    return ys[0] * ys[2] * ys[3]


def wg_exactness_bound(case):
    return wg_rows(case) * XMAX * XMAX + BMAX


def wg_bound(case, ref, A):
    """Gaussian leg, per element of the fp32 gradient: one fp32 ulp of the reference + the running-error bound of M
    fp32 additions in any order (splits, workspace reduce, atomics), times 2, on the absolute-value result."""
    return 2.0 ** -23 * ref.abs() + 2 * wg_rows(case) * U24 * A


# ------------------------------------------------------------------------------------------------------------------
# layouts
# ------------------------------------------------------------------------------------------------------------------
def to_pairs(x4):
    """(N, 4, Hp, Wp) -> the pixel-pair view (N, Hp, Wp / 2, 8): element e * 4 + c of pair (h, q) is x[c][h][2 q + e]."""
    N, _, Hp, Wp = x4.shape
    return x4.permute(0, 2, 3, 1).reshape(N, Hp, Wp // 2, 8).contiguous()


def pair_weight(w):
    """(K, 4, 7, 8) -> (K, 7 * 4 * 8): w'[k][r][j][e * 4 + c] = w[k][c][r][2 j + e]."""
    K = w.shape[0]
    return w.view(K, 4, 7, 4, 2).permute(0, 2, 3, 4, 1).reshape(K, 224).contiguous()


def unpair_weight(wp):
    K = wp.shape[0]
    return wp.view(K, 7, 4, 2, 4).permute(0, 4, 1, 2, 3).reshape(K, 4, 7, 8)
