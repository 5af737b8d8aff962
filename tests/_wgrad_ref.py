"""f64 restatement of the weight-gradient descriptor (include/vaegan_hip.h, vg_wg_desc), the integer operands that make
every summation order give the same f32 bits, and the case table of tests/test_wgrad_cpu.py and tests/test_gpu_wgrad.py.

    dW[np*s_np + cq*s_cq + (a*TW + c)*s_t] = sum_{b,gy,gx} P[b,gy,gx,np] * Q[b, gy*SY + y0 + DY*a, gx*SX + x0 + DX*c, cq]

wgrad_ref is written from that comment and takes a geometry.WGSpec: it knows nothing of torch.nn.grad, of tiles, splits or
slabs.  plan() is the only part that looks at the launcher (csrc/wgrad.hip, vg_wgrad): it names the kernels a case reaches,
so that the case table can be checked for coverage -- if the launcher's rules change, the coverage test fails and the table is
revisited."""
import dataclasses
import importlib

import torch

PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
G = importlib.import_module(PKG + ".geometry")

TORCH_DT = {G.F32: torch.float32, G.BF16: torch.bfloat16}
DT_NAME = {G.F32: "f32", G.BF16: "bf16"}


# ---- the restatement ---------------------------------------------------------------------------------------------------
def _tap_range(n_grid, stride, off, n_img):
    """Grid indices g in [0, n_grid) whose tap row g*stride + off lies inside [0, n_img): a contiguous range."""
    ok = [g for g in range(n_grid) if 0 <= g * stride + off < n_img]
    return (ok[0], ok[-1] + 1) if ok else (0, 0)


def wgrad_ref(spec, P, Q):
    """P [B][GH][GW][PC], Q [B][QH][QW][QC] (any dtype) -> flat f64 dW of NP*s_np elements.  One [NP x M] . [M x NQ]
    product per filter tap over the pixel rows whose tap lies inside the image (out-of-image taps are zero)."""
    P = P.reshape(spec.B, spec.GH, spec.GW, spec.PC)[..., :spec.NP].double()
    Q = Q.reshape(spec.B, spec.QH, spec.QW, spec.QC)[..., :spec.NQ].double()
    dW = torch.zeros(spec.NP * spec.s_np, dtype=torch.float64)
    np_i = torch.arange(spec.NP)[:, None] * spec.s_np
    cq_i = torch.arange(spec.NQ)[None, :] * spec.s_cq
    for a in range(spec.TH):
        y_lo, y_hi = _tap_range(spec.GH, spec.SY, spec.y0 + spec.DY * a, spec.QH)
        for c in range(spec.TW):
            x_lo, x_hi = _tap_range(spec.GW, spec.SX, spec.x0 + spec.DX * c, spec.QW)
            if y_hi <= y_lo or x_hi <= x_lo:
                continue
            iy = torch.arange(y_lo, y_hi) * spec.SY + spec.y0 + spec.DY * a
            ix = torch.arange(x_lo, x_hi) * spec.SX + spec.x0 + spec.DX * c
            p = P[:, y_lo:y_hi, x_lo:x_hi, :].reshape(-1, spec.NP)
            q = Q[:, iy][:, :, ix].reshape(-1, spec.NQ)
            dW[(np_i + cq_i + (a * spec.TW + c) * spec.s_t).flatten()] = (p.T @ q).flatten()
    return dW


# ---- integer operands --------------------------------------------------------------------------------------------------
_VALS = torch.tensor([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0])


def _int_tensor(shape, real, dtype, gen):
    t = torch.zeros(shape)
    t[..., :real] = _VALS[torch.randint(0, 6, tuple(shape[:-1]) + (real,), generator=gen)]
    return t.to(TORCH_DT[dtype])


def int_operands(spec, dtype, seed):
    """-> (P, Q) in the storage dtype: every real channel drawn from {+-1, +-2, +-3} (never 0: a dropped zero term would be
    invisible), every padding channel 0.  The values are exact in bf16, every product is at most 9 and every partial sum is
    an integer of magnitude <= 9 M: below 2^24 they are exact in f32 in ANY order, so every split count, slab order and
    kernel variant must give the same bits.  The factor 2 covers the accumulating call (dW <- dW + dW')."""
    M = spec.B * spec.GH * spec.GW
    assert 2 * 9 * M < 2 ** 24, f"M = {M}: integer sums would leave the exact range of f32"
    gen = torch.Generator().manual_seed(seed)
    P = _int_tensor((spec.B, spec.GH, spec.GW, spec.PC), spec.NP, dtype, gen)
    Q = _int_tensor((spec.B, spec.QH, spec.QW, spec.QC), spec.NQ, dtype, gen)
    return P, Q


def int_dw(spec, seed):
    """A second integer tensor (|x| <= 3) to accumulate onto."""
    gen = torch.Generator().manual_seed(seed)
    return _VALS[torch.randint(0, 6, (spec.NP * spec.s_np,), generator=gen)]


# ---- which kernels a case reaches (restates the launcher's documented choices) -----------------------------------------
def plan(spec, dtype, ws_bytes, wg_spec=3, wg_dma=1, wg_reduce_t=1):
    """nsplit recovered from vg_wgrad_ws_bytes (= nsplit * NPpad * tiles_kq * tile * 4) and the labels of the main and the
    reduce kernel vg_wgrad launches for it under the given VG_WG_SPEC / VG_WG_DMA / VG_WG_REDUCE_T (callers pass a zero
    page, as ops.wgrad does)."""
    tile, srows = (64, 32) if dtype == G.F32 else (128, 64)
    T = spec.TH * spec.TW
    KQ = T * spec.QC
    tiles_kq, tiles_np = -(-KQ // tile), -(-spec.PC // tile)
    slab = tiles_np * tile * tiles_kq * tile * 4
    assert ws_bytes > 0 and ws_bytes % slab == 0, (ws_bytes, slab)
    nsplit = ws_bytes // slab
    M = spec.B * spec.GH * spec.GW
    rps = -(-(-(-M // srows)) // nsplit) * srows                     # whole stages per split
    last = M - (nsplit - 1) * rps
    assert 0 < last <= rps, (M, nsplit, rps)
    if dtype == G.F32:
        main = "f32"
    elif not wg_dma:
        main = "bf16_reg"
    elif wg_spec == 3 and tiles_kq % 2 == 0:
        main = "ws<2,8>"
    elif wg_spec == 2 and tiles_kq % 2 == 0:
        main = "ws<2,4>"
    elif wg_spec != 0:
        main = "ws<1,8>"
    else:
        main = "bf16_dma"
    stream = (wg_reduce_t and T <= 16 and spec.s_t == 1 and spec.s_cq == T and spec.QC % 64 == 0 and spec.NQ == spec.QC
              and spec.s_np % 4 == 0)
    if dtype == G.BF16 and stream and nsplit <= 16 and spec.NP * (spec.QC >> 6) >= 256:
        reduce, SPL = "reduce_t", 0
    else:
        vec = spec.NQ % 4 == 0 and spec.QC % 4 == 0
        VC = 4 if vec else 1
        total = spec.NP * -(-spec.NQ // VC)
        SPL = 32 if nsplit >= 64 else (8 if nsplit >= 8 else 1)
        EL = 256 // SPL
        big = T >= 16 and -(-total // EL) >= 2048
        reduce = f"generic<{16 if big else 4},{VC}> SPL={SPL}"
    return dict(nsplit=nsplit, rows_per_split=rps, last_rows=last, partial_stage=last % srows != 0, T=T, main=main,
                reduce=reduce)


# ---- the case table ----------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    kind: str          # conv | convT | linear (H: side of the map, Cin: C, Cout: N)
    B: int
    H: int
    Cin: int
    Cout: int
    k: int = 0
    s: int = 0
    p: int = 0
    dtypes: tuple = (G.F32, G.BF16)
    target: int = 0    # VG_WG_TARGET, 0: the default

    @property
    def id(self):
        geo = f"{self.kind}-B{self.B}-H{self.H}-{self.Cin}x{self.Cout}"
        return geo + (f"-k{self.k}s{self.s}p{self.p}" if self.kind != "linear" else "") + (f"-t{self.target}" if self.target else "")

    def spec(self, dtype):
        if self.kind == "conv":
            return G.conv_wgrad(self.B, self.H, self.H, self.Cin, self.Cout, self.k, self.s, self.p, dtype)
        if self.kind == "convT":
            return G.convT_wgrad(self.B, self.H, self.H, self.Cin, self.Cout, self.k, self.s, self.p, dtype)
        return G.linear_wgrad(self.B, self.H, self.H, self.Cin, self.Cout, dtype)


_F, _B = (G.F32,), (G.BF16,)
NSPLIT64 = Case("conv", 16, 64, 8, 8, 4, 2, 1)                        # M=16384, nsplit 64, SPL=32; bf16 ws<1,8>
PARTIAL_LAST = Case("conv", 16, 66, 8, 8, 4, 2, 1, _B)                # nsplit 55, SPL=8, last split 144 rows = 2 1/4 stages
REDUCE_T6 = Case("conv", 24, 16, 64, 256, 4, 2, 1, _B)                # reduce_t, nsplit 6 (4 + 2)
REDUCE_T9TAPS = Case("conv", 13, 16, 64, 256, 3, 1, 1, _B)            # reduce_t with T=9, nsplit 13, ws<1,8>
TRANSPOSED = Case("convT", 12, 8, 256, 64, 4, 2, 1, _B)               # reduce_t through the transposed form, nsplit 3
LINEAR36 = Case("linear", 70, 6, 40, 24)                              # 36 taps, 9 tap groups
CASES = [
    NSPLIT64,
    PARTIAL_LAST,
    Case("conv", 16, 64, 3, 32, 4, 2, 0, _F),                         # 31x31 grid, nsplit 54, <4,1> SPL=8, last split 112 rows
    Case("conv", 8, 32, 6, 10, 4, 2, 1, _F),                          # NQ % 4 != 0: <4,1>, SPL=8
    Case("conv", 4, 31, 32, 64, 4, 2, 0, _B),                         # nsplit 3, ws<2,8>, SPL=1, partial last split
    Case("conv", 3, 33, 8, 8, 4, 2, 1),                               # nsplit 3, odd H
    Case("conv", 5, 9, 12, 20, 3, 1, 1),                              # 9 taps: partial tap group in <4,.>; M=405
    Case("conv", 7, 12, 136, 72, 4, 2, 1, _B),                        # odd kq tile count (17), NP not a tile multiple
    Case("conv", 8, 16, 64, 256, 4, 2, 1, _B),                        # reduce_t, nsplit 2
    REDUCE_T6,
    Case("conv", 40, 16, 64, 256, 4, 2, 1, _B),                       # reduce_t, nsplit 10
    REDUCE_T9TAPS,
    TRANSPOSED,
    Case("linear", 300, 2, 256, 200, dtypes=_B),                      # reduce_t T=4, M=300 (partial stage)
    Case("linear", 300, 1, 256, 300, dtypes=_B),                      # reduce_t T=1
    LINEAR36,
    Case("conv", 2, 64, 512, 512, 4, 2, 1, _F, 8192),                 # <16,4>, SPL=8
    Case("conv", 16, 64, 130, 128, 4, 2, 1, _F, 8192),                # <16,1>, SPL=32
]
CASE_PARAMS = [(c, dt) for c in CASES for dt in c.dtypes]

# the non-default builds of the same result: a subset of the table under every weight-gradient switch
SWITCH_CASES = [NSPLIT64, PARTIAL_LAST, REDUCE_T6, REDUCE_T9TAPS, TRANSPOSED, LINEAR36]
SWITCHES = [("VG_WG_SPEC", 0), ("VG_WG_SPEC", 1), ("VG_WG_SPEC", 2), ("VG_WG_DMA", 0), ("VG_WG_REDUCE_T", 0),
            ("VG_WG_TARGET", 64), ("VG_WG_TARGET", 4096), ("VG_WG_XCD", 2)]
_F32_SWITCHES = ("VG_WG_TARGET", "VG_WG_XCD")                        # the f32 kernel reads only these two
SWITCH_PARAMS = [(c, dt, name, val) for c in SWITCH_CASES for dt in c.dtypes for name, val in SWITCHES
                 if dt == G.BF16 or name in _F32_SWITCHES]
CASE_IDS = [f"{c.id}-{DT_NAME[dt]}" for c, dt in CASE_PARAMS]
SWITCH_IDS = [f"{c.id}-{DT_NAME[dt]}-{name}={val}" for c, dt, name, val in SWITCH_PARAMS]
