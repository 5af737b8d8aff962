"""f64 reference of the gather-GEMM (include/vaegan_hip.h, vg_gg_desc) through torch's own convolutions, the integer operands
that make every summation order give the same f32 bits, and the case table of tests/test_gg_cpu.py and tests/test_gpu_gg.py.

The OUTPUT reference is torch's conv2d / conv_transpose2d / linear / torch.nn.grad.conv2d_input in f64 on the layer's NCHW
tensors: it knows nothing of geometry.py, of the operand packer or of the descriptor, so a case checks all three together with
the kernel.  Only two things are taken from the descriptor, as the header states them: which output pixels a launch writes
(written_mask) and which rows feed which BatchNorm statistics slab (stats_ref: slab row phase * m_tiles + m / bm with
m = (b * GH + gy) * GW + gx, sums of the UNROUNDED f32 values, bias included, over valid output pixels).

label() names the kernel a plan (ops.gather_gemm_plan, i.e. the record vg_gather_gemm launches from) stands for; every row of
the table carries the label of the branch it is there for, and both test files assert it against the built library."""
import dataclasses
import importlib

import torch
import torch.nn.functional as F

from _emulate import to_nhwc

PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
G = importlib.import_module(PKG + ".geometry")

TORCH_DT = {G.F32: torch.float32, G.BF16: torch.bfloat16, G.FP8: torch.bfloat16}     # fp8 operands are cast on the device
DT_NAME = {G.F32: "f32", G.BF16: "bf16", G.FP8: "fp8"}
RELU, LRELU = 1, 2
ACT_SLOPE, MASK_SLOPE = 0.25, 0.5                       # powers of two: slope * (an integer below 2^24) is exact in f32
EXACT = 2 ** 24
BIG = "2000000000"
# every case runs under these (small problems take the large tiles; the 8-wave patch tiles only where a row asks for them)
BASE_ENV = (("VG_TILE_MIN_WGS", "1"), ("VG_GG_PHASE4_MIN", "1"), ("VG_PATCH256_MIN", BIG), ("VG_PATCH256X64_MIN", BIG))


# ---- the case table's row -----------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    label: str          # the kernel this row is there for: label(plan) must equal it
    kind: str           # conv | convT | conv_dgrad | convT_dgrad | linear | linear_dgrad; the LAYER is (Cin -> Cout) on an H x H input
    B: int
    H: int
    Cin: int
    Cout: int
    k: int = 4
    s: int = 2
    p: int = 1
    dtype: int = G.BF16
    epi: str = ""       # '+'-joined: b bias, s statistics, r ReLU, l LeakyReLU, mr / ml activation-backward mask (ReLU / LeakyReLU)
    vals: int = 3       # operands from {+-1 .. +-vals}
    env: tuple = ()     # switches on top of BASE_ENV

    @property
    def id(self):
        geo = f"{self.kind}-B{self.B}-H{self.H}-{self.Cin}x{self.Cout}"
        if not self.kind.startswith("linear"):
            geo += f"-k{self.k}s{self.s}p{self.p}"
        sw = "".join(f"-{n[3:]}={'big' if v == BIG else v}" for n, v in self.env)
        return f"{DT_NAME[self.dtype]}-{geo}{'-' + self.epi if self.epi else ''}{sw}"

    @property
    def switches(self):
        d = dict(BASE_ENV)
        d.update(self.env)
        return d

    def has(self, e):
        return e in self.epi.split("+")

    @property
    def act(self):
        return (RELU, 0.0) if self.has("r") else (LRELU, ACT_SLOPE) if self.has("l") else None

    @property
    def mask(self):
        return (RELU, 0.0) if self.has("mr") else (LRELU, MASK_SLOPE) if self.has("ml") else None

    def specs(self):
        """-> (GGSpec, PackSpec) of the storage dtype (fp8 operands ride the bf16 geometry, as in the engines)."""
        dt = G.BF16 if self.dtype == G.FP8 else self.dtype
        a = (self.B, self.H, self.H, self.Cin, self.Cout, self.k, self.s, self.p, dt)
        if self.kind == "linear":
            return G.linear_fprop(self.B, self.H, self.H, self.Cin, self.Cout, dt)
        if self.kind == "linear_dgrad":
            return G.linear_dgrad(self.B, self.H, self.H, self.Cin, self.Cout, dt)
        return {"conv": G.conv_fprop, "convT": G.convT_fprop, "conv_dgrad": G.conv_dgrad, "convT_dgrad": G.convT_dgrad}[self.kind](*a)

    # shapes of the layer-level (NCHW) operands: the gathered tensor, the parameter, and the real output channels
    def x_shape(self):
        if self.kind in ("conv", "convT", "linear"):
            return (self.B, self.Cin, self.H, self.H)
        if self.kind == "conv_dgrad":
            o = G.conv_out(self.H, self.k, self.s, self.p)
            return (self.B, self.Cout, o, o)
        if self.kind == "convT_dgrad":
            o = G.convT_out(self.H, self.k, self.s, self.p)
            return (self.B, self.Cout, o, o)
        return (self.B, self.Cout, 1, 1)

    def w_shape(self):
        if self.kind in ("conv", "conv_dgrad"):
            return (self.Cout, self.Cin, self.k, self.k)
        if self.kind in ("convT", "convT_dgrad"):
            return (self.Cin, self.Cout, self.k, self.k)
        return (self.Cout, self.Cin * self.H * self.H)


def core(case, x, w):
    """The layer's linear map in f64, NCHW in, NCHW out, no bias: torch's own operators."""
    x, w = x.double(), w.double()
    if case.kind == "conv":
        return F.conv2d(x, w, None, stride=case.s, padding=case.p)
    if case.kind == "convT":
        return F.conv_transpose2d(x, w, None, stride=case.s, padding=case.p)
    if case.kind == "conv_dgrad":
        return torch.nn.grad.conv2d_input((case.B, case.Cin, case.H, case.H), w, x, stride=case.s, padding=case.p)
    if case.kind == "convT_dgrad":             # the input gradient of a transposed convolution IS the convolution with its weight
        return F.conv2d(x, w, None, stride=case.s, padding=case.p)
    if case.kind == "linear":
        return F.linear(x.flatten(1), w)[:, :, None, None]
    return (x.flatten(1) @ w).view(case.B, case.Cin, case.H, case.H)          # linear_dgrad: dh = dout . W


def to_output_layout(g, y):
    """NCHW f64 result -> [B][OH][OW][N] as the descriptor lays it out.  The two 'taps folded into N' forms (Linear data
    gradient, ConvTranspose2d on a 1 x 1 input) write the NHWC map of one image as the N columns of one pixel."""
    y = y.permute(0, 2, 3, 1).contiguous()
    if g.OH == 1 and g.OW == 1:
        y = y.reshape(g.B, 1, 1, -1)
    assert tuple(y.shape) == (g.B, g.OH, g.OW, g.N), (tuple(y.shape), (g.B, g.OH, g.OW, g.N))
    return y


# ---- integer operands --------------------------------------------------------------------------------------------------
def _ints(shape, vals, gen):
    """Integers from {+-1 .. +-vals}, never 0: a dropped zero term would be invisible."""
    v = torch.randint(1, vals + 1, shape, generator=gen).double()
    return v * (torch.randint(0, 2, shape, generator=gen).double() * 2 - 1)


def operands(case, seed=1):
    """-> dict(x NCHW f64, w f64 in the parameter layout, bias f64 [N] or None, mask f64 [B][OH][OW][OC] or None).
    x and w hold +-1 .. +-vals in every element (exact in bf16, and +-1 exact in e4m3 after the weights' * 2^6); the bias
    holds integers of [-4, 4]; the mask tensor integers of [-2, 2], zeros included (they sit on the '> 0' boundary)."""
    g, _ = case.specs()
    gen = torch.Generator().manual_seed(seed)
    assert case.dtype != G.FP8 or case.vals == 1, "fp8: +-1 is the one operand family the MFMA is pinned exact on"
    x = _ints(case.x_shape(), case.vals, gen)
    w = _ints(case.w_shape(), case.vals, gen)
    bias = torch.randint(-4, 5, (g.N,), generator=gen).double() if case.has("b") else None
    mask = torch.randint(-2, 3, (g.B, g.OH, g.OW, g.OC), generator=gen).double() if case.mask else None
    return dict(x=x, w=w, bias=bias, mask=mask)


def x_nhwc(case, x):
    """The gathered operand as the kernel reads it: NHWC, padding channels zero, storage dtype (bf16 for fp8 cases: cast on
    the device by vg_cast_fp8, as in the product)."""
    g, _ = case.specs()
    return to_nhwc(x, g.IC).to(TORCH_DT[case.dtype]).contiguous()


# ---- the epilogue, restated ----------------------------------------------------------------------------------------------
def _round(y, dtype):
    """f64 (exactly representable in f32: asserted by exactness()) -> the output dtype: round-to-nearest-even to bf16 for bf16
    and fp8 operands, nothing for f32."""
    y = y.float()
    return y if dtype == G.F32 else y.to(torch.bfloat16)


def _apply(y, x, act):
    code, slope = act
    return torch.where(x > 0, y, y * slope if code == LRELU else torch.zeros_like(y))


def output_ref(case, ops_, yf):
    """yf: [B][OH][OW][N] f64, bias included -> Y [B][OH][OW][OC] in the output dtype: activation in f32, rounding, then the
    mask on the rounded value (rounded again), zeros in the padding channels [N, OC)."""
    g, _ = case.specs()
    y = yf if case.act is None else _apply(yf, yf, case.act)
    Y = torch.zeros(g.B, g.OH, g.OW, g.OC, dtype=torch.float32 if case.dtype == G.F32 else torch.bfloat16)
    Y[..., :g.N] = _round(y, case.dtype)
    if case.mask is not None:
        Y = _round(_apply(Y.double(), ops_["mask"], case.mask), case.dtype)
    return Y


def preact_ref(case, ops_):
    """[B][OH][OW][N] f64: the accumulators plus bias, before activation and rounding (what the statistics are formed from)."""
    g, _ = case.specs()
    y = to_output_layout(g, core(case, ops_["x"], ops_["w"]))
    return y if ops_["bias"] is None else y + ops_["bias"]


def written_mask(g):
    """[B][OH][OW] int32: how many (phase, grid pixel) pairs write each output pixel; pairs that fall outside are skipped."""
    wr = torch.zeros(g.B, g.OH, g.OW, dtype=torch.int32)
    for p in range(g.nphase):
        oy = torch.arange(g.GH) * g.OSY + g.ooy[p]
        ox = torch.arange(g.GW) * g.OSX + g.oox[p]
        wr[:, oy[oy < g.OH][:, None], ox[ox < g.OW][None, :]] += 1
    return wr


def skipped_pairs(g):
    """Number of (phase, gy, gx) triples of one image whose output pixel lies outside the tensor."""
    n = 0
    for p in range(g.nphase):
        vy = int(((torch.arange(g.GH) * g.OSY + g.ooy[p]) < g.OH).sum())
        vx = int(((torch.arange(g.GW) * g.OSX + g.oox[p]) < g.OW).sum())
        n += g.GH * g.GW - vy * vx
    return n


def stats_ref(g, yf, bm, fn=None):
    """-> [nphase * m_tiles][2][N] f64: per slab (sum y, sum y^2) over the slab's valid rows.  fn: applied to y first (abs for
    the exactness condition)."""
    M = g.B * g.GH * g.GW
    mt = -(-M // bm)
    out = torch.zeros(g.nphase * mt, 2, g.N, dtype=torch.float64)
    for p in range(g.nphase):
        oy = torch.arange(g.GH) * g.OSY + g.ooy[p]
        ox = torch.arange(g.GW) * g.OSX + g.oox[p]
        oy, ox = oy[oy < g.OH], ox[ox < g.OW]                        # (a prefix of the grid: the offsets only grow)
        v = torch.zeros(mt * bm, g.N, dtype=torch.float64)
        grid = v[:M].view(g.B, g.GH, g.GW, g.N)
        grid[:, :oy.numel(), :ox.numel()] = yf[:, oy][:, :, ox]
        if fn is not None:
            v = fn(v)
        v = v.view(mt, bm, g.N)
        out[p * mt:(p + 1) * mt, 0] = v.sum(1)
        out[p * mt:(p + 1) * mt, 1] = (v * v).sum(1)
    return out


def exactness(case, ops_, yf, bm):
    """The conditions under which f32 adds every term exactly in ANY order -> list of violated ones (empty: exact).
    Per output: (number of real products) * vals^2 + |bias| bounds sum |x||w| + |bias| from above."""
    g, _ = case.specs()
    bad = []
    products = g.TH * g.TW * case.x_shape()[1]
    bound = products * case.vals ** 2 + (0 if ops_["bias"] is None else int(ops_["bias"].abs().max()))
    if not bound < EXACT:
        bad.append(f"per output: {bound} >= 2^24")
    if case.has("s"):
        s_abs = stats_ref(g, yf, bm, fn=torch.abs)
        if not float(s_abs[:, 0].max()) < EXACT:
            bad.append(f"slab sum |y| = {float(s_abs[:, 0].max())} >= 2^24")
        if not float(s_abs[:, 1].max()) < EXACT:
            bad.append(f"slab sum y^2 = {float(s_abs[:, 1].max())} >= 2^24")
    return bad


# ---- naming a plan -----------------------------------------------------------------------------------------------------
def label(p):
    """The kernel (template instantiation) a plan of ops.gather_gemm_plan launches, and the reduce that follows a split."""
    if p["family"] == "narrowk":
        return f"ggn<{p['detail'][0]},{p['detail'][1]}>"
    if p["family"] == "phase4":
        return f"ggq<{p['bn']},{p['detail'][0]}>"
    if p["family"] == "patch":
        wm, bn, nr = p["bm"] // 64, p["bn"], p["detail"][1]
        return "ggp<" + ",".join(str(a) for a in ((wm,) if bn == 128 else (wm, bn) if nr == 0 else (wm, bn, nr))) + ">"
    s = f"gg {p['bm']}x{p['bn']} {'dma' if p['dma'] else 'reg'}"
    return s + (f" splitk-{p['reduce']}" if p["ksplit"] > 1 else "")


# ---- the case table ----------------------------------------------------------------------------------------------------
_F, _B, _8 = G.F32, G.BF16, G.FP8
REG = (("VG_GG_DMA", "0"),)
T64 = (("VG_TILE_MIN_WGS", BIG),)                       # no larger tile offers enough workgroups: 64 x 64
T128x64 = (("VG_TILE_MIN_WGS", "10"),)                  # for the ragged shape below: 8 tiles of 128 x 128, 12 of 128 x 64
P256 = (("VG_PATCH256_MIN", "1"), ("VG_PATCH256X64_MIN", "1"))
GENERAL = (("VG_SPLITK_GENERAL", "1"),)


def _ragged(lab, dtype, Cin, Cout, epi, env=()):
    """3 x 3 convolution of a 9 x 9 map, 5 images: M = 405 (no multiple of any tile), Cout 130 / 26 / 10 (no multiple of the
    tile's columns, and OC > N in both dtypes).  Cin 32: 9 (bf16) K chunks, whole chunks per tap -- the last stage of every
    2- and 4-chunk stage is partial; Cin 20: a tap is no whole chunk (the per-unit address path of the DMA ring) and
    Kp = 224 (bf16) / 192 (f32) > K = 216 / 180."""
    return Case(lab, "conv", 5, 9, Cin, Cout, 3, 1, 1, dtype, epi, env=env)


GENERIC = [
    # f32 (register-staged v_mfma_f32_16x16x4_f32): every tile
    _ragged("gg 128x128 reg", _F, 20, 130, "b+s"), _ragged("gg 128x128 reg", _F, 32, 130, "mr"),
    _ragged("gg 128x64 reg", _F, 32, 130, "b+l", T128x64), _ragged("gg 128x64 reg", _F, 20, 130, "s", T128x64),
    _ragged("gg 64x64 reg", _F, 20, 130, "b+ml", T64), _ragged("gg 64x64 reg", _F, 32, 130, "b+s", T64),
    _ragged("gg 128x32 reg", _F, 32, 26, "b+r"), _ragged("gg 128x32 reg", _F, 20, 26, "s"),
    _ragged("gg 256x16 reg", _F, 20, 10, "b+s"), _ragged("gg 256x16 reg", _F, 32, 10, "ml"),
    # bf16 on the LDS-DMA ring
    _ragged("gg 128x128 dma", _B, 32, 130, "b+s"), _ragged("gg 128x128 dma", _B, 20, 130, "l"),
    _ragged("gg 128x64 dma", _B, 20, 130, "b+ml", T128x64), _ragged("gg 128x64 dma", _B, 32, 130, "s", T128x64),
    _ragged("gg 64x64 dma", _B, 32, 130, "mr", T64), _ragged("gg 64x64 dma", _B, 20, 130, "b+s", T64),
    # bf16 register-staged
    _ragged("gg 128x128 reg", _B, 20, 130, "b+s", REG), _ragged("gg 128x128 reg", _B, 32, 130, "ml", REG),
    _ragged("gg 128x64 reg", _B, 32, 130, "b+r", T128x64 + REG), _ragged("gg 128x64 reg", _B, 20, 130, "s", T128x64 + REG),
    _ragged("gg 64x64 reg", _B, 20, 130, "b+l", T64 + REG), _ragged("gg 64x64 reg", _B, 32, 130, "b+s", T64 + REG),
    # the narrow tiles are register-staged in either dtype
    _ragged("gg 128x32 reg", _B, 32, 26, "b+s"), _ragged("gg 128x32 reg", _B, 20, 26, "ml"),
    _ragged("gg 256x16 reg", _B, 20, 10, "b+l"), _ragged("gg 256x16 reg", _B, 32, 10, "s"),
    # no padding: the last tap column of the last grid column is INSIDE the image (with padding 1 it is a zero tap anyway)
    Case("gg 128x128 dma", "conv", 5, 11, 32, 130, 3, 1, 0, _B, "s"),
    Case("gg 64x64 reg", "conv", 5, 11, 20, 130, 3, 1, 0, _B, "b", env=T64 + REG),
    Case("gg 128x64 reg", "conv", 5, 20, 32, 130, 4, 2, 0, _F, "b+s", env=T128x64),
    # the other descriptor forms on the generic tiles
    Case("gg 128x32 reg", "conv_dgrad", 3, 9, 24, 40, 4, 2, 1, _B, "b+s"),           # odd map: 5 x 5 grid, the last row / column of 3 phases is skipped
    Case("gg 64x64 dma", "conv_dgrad", 3, 9, 70, 40, 4, 2, 1, _B, "s", env=T64),      # the same on the DMA ring, two column tiles
    Case("gg 128x128 reg", "conv_dgrad", 3, 9, 70, 40, 4, 2, 1, _F, "b+s"),
    Case("gg 128x64 dma", "conv_dgrad", 3, 7, 40, 24, 3, 1, 1, _B, "s"),              # stride-1 transposed form: taps walk backwards (DY = -1)
    Case("gg 128x64 dma", "convT", 3, 5, 24, 40, 3, 1, 1, _B, "b+l"),
    Case("gg 128x128 dma", "convT", 8, 1, 100, 64, 4, 1, 0, _B, "b"),                 # 1 x 1 input: taps folded into N = 1024
    Case("gg 128x128 reg", "linear_dgrad", 6, 3, 16, 40, dtype=_F),                   # Linear data gradient: N = 9 * 16
    Case("gg 128x128 dma", "linear_dgrad", 6, 3, 16, 40, dtype=_B, epi="ml"),
]

NARROWK = [  # 3-channel input (IC = 8); 11 x 11 output maps of 3 images: M = 363, the second workgroup holds 107 of 256 rows
    Case("ggn<1,3>", "conv", 3, 11, 3, 16, 3, 1, 1, _B, "b+s"),
    Case("ggn<4,3>", "conv", 3, 11, 3, 64, 3, 1, 1, _B, "l"),
    Case("ggn<4,4>", "conv", 3, 22, 3, 64, 4, 2, 1, _B, "b+l"),                       # stride 2, padding 1
    Case("ggn<4,4>", "conv", 3, 24, 3, 64, 4, 2, 0, _B, "s"),                         # stride 2, padding 0
    Case("ggn<1,4>", "conv", 3, 24, 3, 16, 4, 2, 0, _B, "b+r"),
    Case("ggn<1,4>", "conv", 3, 22, 2, 16, 4, 2, 1, _B, "b+s"),
]

PHASE4 = [  # k4 s2 p1 transposed form, <= 32 output channels: all four phases of 256 grid pixels per workgroup
    Case("ggq<16,7>", "convT", 2, 16, 32, 12, epi="b+s"),                             # 16 x 16 grid, 12 real columns
    Case("ggq<32,7>", "convT", 8, 8, 64, 24, epi="b+l"),                              # 8 x 8 grid: 4 images per tile, 24 real columns
    Case("ggq<32,7>", "conv_dgrad", 2, 32, 32, 64, epi="ml"),                         # 16 x 16 grid through the data gradient
    Case("ggq<16,9>", "convT", 32, 4, 32, 16, epi="s"),                               # 4 x 4 grid: 16 images per tile
    Case("ggq<32,9>", "convT", 32, 4, 96, 32, epi="b+r"),
    Case("ggq<32,9>", "convT", 16, 4, 64, 24, epi="b+s"),
    Case("ggq<16,9>", "conv_dgrad", 1, 256, 16, 32, epi="mr"),                        # 128-wide grid: a tile is two grid rows
    Case("ggq<32,9>", "convT", 1, 128, 32, 24, epi="b+s"),
]

PATCH = [  # 2 x 2-tap phases of the transposed form / the direct k4 s2 convolution, input patch resident in LDS
    Case("ggp<2>", "convT", 4, 8, 32, 72, epi="b+s"),                                 # transposed, 8 x 8 grid: 2 images per tile
    Case("ggp<2>", "conv", 1, 32, 32, 130, epi="b+l"),                                # direct, 16 x 16 grid: a tile is 8 of 16 rows; 2 column tiles
    Case("ggp<2>", "conv_dgrad", 2, 32, 72, 32, epi="ml"),
    Case("ggp<4>", "convT_dgrad", 2, 16, 130, 32, epi="s", env=P256),                 # direct, 256-row tile = one image
    Case("ggp<4>", "convT", 2, 32, 32, 72, epi="b+r", env=P256),                      # transposed, 32 x 32 grid: a tile is 8 of 32 rows
    Case("ggp<4>", "conv_dgrad", 2, 32, 72, 32, epi="ml", env=P256),                  # transposed, 16 x 16 grid, the mask on the 8-wave tile
    Case("ggp<4,64>", "convT", 8, 8, 64, 40, epi="b+s", env=P256),                    # 4 images per tile
    Case("ggp<4,64>", "conv", 2, 64, 32, 64, epi="mr", env=P256),                     # direct, a tile is 8 of 32 rows
    Case("ggp<2,64>", "convT", 16, 4, 32, 48, epi="b+s"),                             # 4 x 4 grid: 8 images, 200 patch pixels
    Case("ggp<2,64>", "convT_dgrad", 1, 64, 40, 32, epi="l"),                         # direct, 64-wide grid: 195 patch pixels
    Case("ggp<2,64,3>", "conv", 2, 32, 32, 64, epi="b+s"),                            # 153 patch pixels: three DMA rounds
    Case("ggp<2,64,3>", "conv_dgrad", 4, 16, 40, 64, epi="b+ml"),                     # transposed, 8 x 8 grid: 2 images
    Case("ggp<2,32>", "conv", 1, 64, 32, 32, epi="b+s"),                              # direct, 32-wide grid, exactly 32 columns
    Case("ggp<2,32>", "convT_dgrad", 8, 8, 32, 64, epi="mr"),
    Case("ggp<2,32>", "conv_dgrad", 2, 16, 32, 64, epi="b+ml"),                       # transposed, 8 x 8 grid: 128 rows (no 4-phase tile), sub-pixel scatter
]

SPLITK = [
    # flat form: Linear layers, no statistics.  K = 16 * 64: 16 two-chunk stages -> 4 slices (the reduce's tail loop only)
    Case("gg 128x128 dma splitk-flat", "linear", 8, 4, 64, 100, epi="b"),
    Case("gg 128x128 reg splitk-flat", "linear", 8, 4, 64, 100, epi="b", env=REG),
    Case("gg 128x128 reg splitk-flat", "linear", 8, 4, 64, 100, dtype=_F, epi="b"),   # f32: 64 stages -> 16 slices (two unrolled rounds)
    Case("gg 64x64 dma splitk-flat", "linear", 8, 4, 64, 100, epi="b", env=T64),      # 8 four-chunk stages -> 4 slices of 2
    # K = 4 * 672: 42 stages -> 9 slices of 5, the last one holds 2 (one unrolled round of the reduce + its tail)
    Case("gg 128x128 dma splitk-flat", "linear", 5, 2, 672, 100, epi="b"),
    Case("gg 128x128 reg splitk-flat", "linear", 5, 2, 672, 100, env=REG),
    Case("gg 128x128 reg splitk-flat", "linear", 5, 2, 672, 100, dtype=_F, epi="b"),
    Case("gg 128x64 dma splitk-flat", "linear", 5, 2, 672, 40, epi="b"),
    # general form: 64 x 64 tiles with sub-pixel phases / statistics, reduced per tile (bias, OC > N)
    Case("gg 64x64 dma splitk-tile", "convT", 2, 4, 256, 68, epi="b+s", env=T64 + GENERAL),
    Case("gg 64x64 reg splitk-tile", "convT", 2, 4, 256, 68, epi="b+s", env=T64 + GENERAL + REG),
    Case("gg 64x64 dma splitk-tile", "conv", 3, 6, 64, 70, 4, 2, 0, epi="b+s", env=T64 + GENERAL),
    Case("gg 64x64 dma splitk-tile", "convT", 2, 4, 256, 68, epi="b", env=T64 + GENERAL),
    # big-K form: the data gradient of ConvTranspose2d(1024 -> 128) at B = 64 on a 4 x 4 input, 64 tiles of 128 x 128
    Case("gg 128x128 dma splitk-flat", "convT_dgrad", 64, 4, 1024, 128),
]

FP8 = [  # +-1 operands; weights through vg_cast_fp8(., 6)
    Case("gg 128x128 dma", "conv", 3, 16, 64, 130, dtype=_8, epi="s", vals=1),
    Case("gg 128x128 reg", "conv", 3, 16, 64, 130, dtype=_8, epi="b+l", vals=1, env=REG),
    Case("gg 128x64 dma", "convT", 3, 8, 128, 40, dtype=_8, epi="b+s", vals=1),       # four phases
    Case("gg 128x64 reg", "convT", 3, 8, 128, 40, dtype=_8, epi="b+r", vals=1, env=REG),
    Case("gg 64x64 dma", "conv", 3, 10, 16, 70, dtype=_8, epi="b", vals=1, env=T64),
    Case("gg 64x64 reg", "conv", 3, 10, 16, 70, dtype=_8, epi="b+s", vals=1, env=T64 + REG),
]

CASES = GENERIC + NARROWK + PHASE4 + PATCH + SPLITK + FP8

# VG_GG_NMAJOR: forced on for every launch whose n-tile count is a multiple of 8 (=2) and off (=0); pure placement
_NM8 = [Case("gg 64x64 dma", "conv", 2, 5, 32, 512, 3, 1, 1, epi="b+s", env=T64),                 # 8 column tiles, 1 row tile
        Case("gg 128x128 dma", "convT", 8, 1, 100, 64, 4, 1, 0, epi="b"),                           # 8 column tiles (on by default: weights > input)
        Case("ggp<2>", "convT", 4, 8, 32, 1024, epi="s")]                                            # the patch kernel's own order
_NM3 = [_ragged("gg 64x64 dma", _B, 32, 130, "b+s", T64)]                                            # 3 column tiles: the switch must not apply
SWITCH_CASES = [dataclasses.replace(c, env=c.env + (("VG_GG_NMAJOR", v),)) for c in _NM8 + _NM3 for v in ("0", "2")]
NMAJOR_TILES8 = {c.id for c in SWITCH_CASES[:2 * len(_NM8)]}

ALL_CASES = CASES + SWITCH_CASES
ALL_IDS = [c.id for c in ALL_CASES]
assert len(set(ALL_IDS)) == len(ALL_IDS), "duplicate case ids"


# ---- the launches of the three networks ----------------------------------------------------------------------------------
# (S, B, dtype name of nets.py) of the four benchmarked shapes; S = 256 in both operand dtypes
NETWORK_SHAPES = ((64, 128, "bf16"), (64, 128, "fp32"), (128, 64, "bf16"), (256, 32, "bf16"), (256, 32, "fp8"))


def build_networks(S, dtype):
    """The Encoder, Generator and Discriminator of the benchmark on the CPU: their engines answer geometry questions host only."""
    nets = importlib.import_module(PKG + ".nets")
    return (("E", nets.Encoder([3, S, S], 100, dtype=dtype)), ("G", nets.Generator(nz=100, img_size=S, dtype=dtype)),
            ("D", nets.Discriminator(img_size=S, dtype=dtype)))


def network_launches(S, B, dtype):
    """Every vg_gather_gemm launch a training iteration of the three networks can issue at this shape, as engine.py's forward /
    backward issue them (fused activation of a BatchNorm-less stage, statistics of a BatchNorm stage, the mask of the stage
    below on a data gradient; the stages on the edge-layer kernels launch no gather-GEMM) -- the Discriminator also at 2B,
    the grouped pass.  -> [(key, GGSpec, kernel dtype, dict(bias, want_stats, act, mask))], host only."""
    out = []
    for name, m in build_networks(S, dtype):
        eng = m._engine
        for nb in ((B, 2 * B) if name == "D" else (B,)):
            for i, st in enumerate(eng.stages):
                if st.kind == "head":
                    continue
                if eng.tn(i, nb, "fprop") is None:
                    g, pk = eng.spec(i, nb, "fprop")
                    fuse_act = st.bn is None and st.act != 0
                    epi = dict(bias=st.kind == "linear2" or st.has_bias, want_stats=st.bn is not None and not pk.tap_in_n,
                               act=(st.act, st.slope) if fuse_act else None, mask=None)
                    out.append((f"{name}.{i}.fprop.B{nb}", g, G.FP8 if eng.fp8_ok(i) else eng.dtype, epi))
                if eng.tn(i, nb, "dgrad") is None:
                    g, _ = eng.spec(i, nb, "dgrad")
                    mask = None
                    if i > 0:
                        pst = eng.stages[i - 1]
                        if pst.bn is None and pst.act != 0 and g.N == pst.cout and g.OC == G.padc(pst.cout, eng.dtype):
                            mask = (pst.act, pst.slope)
                    out.append((f"{name}.{i}.dgrad.B{nb}", g, eng.dtype, dict(bias=False, want_stats=False, act=None, mask=mask)))
    return out


def group_stages(S, B, dtype, groups=2):
    """The BatchNorm stages of the Discriminator for a grouped pass of groups * B images (engine.StackEngine.can_group): ->
    [(stage, GGSpec, kernel dtype, rows per group, single-phase plain convolution)], host only."""
    eng = dict(build_networks(S, dtype))["D"]._engine
    out = []
    for i, st in enumerate(eng.stages):
        if st.kind != "head" and st.bn is not None:
            g, pk = eng.spec(i, B * groups, "fprop")
            out.append((i, g, G.FP8 if eng.fp8_ok(i) else eng.dtype, B * st.hout * st.hout, g.nphase == 1 and not pk.tap_in_n))
    return out
