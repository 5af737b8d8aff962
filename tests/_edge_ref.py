"""f64 restatements of the two edge-layer descriptors (include/vaegan_hip.h, vg_tn_desc and vg_ew_desc), integer operands
that make every summation order give the same f32 bits, and the case tables of tests/test_edge_cpu.py and
tests/test_gpu_edge.py.

    vg_tnconv      Y[b][oy][ox][n] = sum_{c,kh,kw} X[b][iy][ix][c] * W[c][n][kh][kw],   oy = iy*S - P + kh,  ox = ix*S - P + kw
    vg_edge_wgrad  dW[c*s_c + n*s_n + kh*K + kw] = sum_{b,py,px} Wd[b][py][px][c] * Nr[b][py*S - P + kh][px*S - P + kw][n]

Both references are written from those two comments, tap by tap: they know nothing of torch's convolutions, of tiles, halo
windows or workgroup walks.  Which kernel instantiation and which tiling a row reaches is not restated here either: every
row carries the fields of the launcher's own plan record (vg_tnconv_plan / vg_edge_wgrad_plan) that it is there for, the
tests compare them with the record before anything else, and a row's `why` names the facet it covers -- if the planner's
rules change, those comparisons fail and the table is revisited."""
import dataclasses
import math

import torch

from _wgrad_ref import G, _VALS, _int_tensor


# ---- the restatements ------------------------------------------------------------------------------------------------------
def tnconv_ref(tn, X, W):
    """X [B][IH][IW][C], W [C][N][K][K] (any dtype) -> f64 Y [B][N][OH][OW] (the layout of Y_nchw).  The scatter form of the
    header: every input pixel adds its N-vector X[pix][:] . W[:, :, kh, kw] to output pixel (iy*S - P + kh, ix*S - P + kw);
    the map is built unpadded and the P border rows and columns are cut off at the end."""
    X = X.reshape(tn.B, tn.IH, tn.IW, tn.C).double()
    W = W.reshape(tn.C, tn.N, tn.K, tn.K).double()
    FH, FW = (tn.IH - 1) * tn.S + tn.K, (tn.IW - 1) * tn.S + tn.K
    assert FH - 2 * tn.P == tn.OH and FW - 2 * tn.P == tn.OW
    full = torch.zeros(tn.B, FH, FW, tn.N, dtype=torch.float64)
    for kh in range(tn.K):
        for kw in range(tn.K):
            full[:, kh:kh + (tn.IH - 1) * tn.S + 1:tn.S, kw:kw + (tn.IW - 1) * tn.S + 1:tn.S] += X @ W[:, :, kh, kw]
    return full[:, tn.P:tn.P + tn.OH, tn.P:tn.P + tn.OW].permute(0, 3, 1, 2).contiguous()


def edge_wgrad_ref(ew, wide, narrow):
    """wide [B][WH][WW][C], narrow [B][NH][NW][8] (any dtype) -> flat f64 dW of C*s_c elements.  One [C x M] . [M x N] product
    per tap over the wide pixels; narrow pixels outside the image are zero."""
    Wd = wide.reshape(ew.B, ew.WH, ew.WW, ew.C).double()
    Nr = narrow.reshape(ew.B, ew.NH, ew.NW, -1)[..., :ew.N].double()
    hi_y = max(0, (ew.WH - 1) * ew.S - ew.P + ew.K - ew.NH)          # rows / columns the last taps reach beyond the image
    hi_x = max(0, (ew.WW - 1) * ew.S - ew.P + ew.K - ew.NW)
    pad = torch.zeros(ew.B, ew.P + ew.NH + hi_y, ew.P + ew.NW + hi_x, ew.N, dtype=torch.float64)
    pad[:, ew.P:ew.P + ew.NH, ew.P:ew.P + ew.NW] = Nr
    dW = torch.zeros(ew.C * ew.s_c, dtype=torch.float64)
    idx = torch.arange(ew.C)[:, None] * ew.s_c + torch.arange(ew.N)[None, :] * ew.s_n
    A = Wd.reshape(-1, ew.C).T
    for kh in range(ew.K):
        for kw in range(ew.K):
            nr = pad[:, kh:kh + (ew.WH - 1) * ew.S + 1:ew.S, kw:kw + (ew.WW - 1) * ew.S + 1:ew.S]
            dW[(idx + kh * ew.K + kw).flatten()] = (A @ nr.reshape(-1, ew.N)).flatten()
    return dW


# ---- integer operands ------------------------------------------------------------------------------------------------------
def tn_operands(tn, seed):
    """-> (X bf16 [B][IH][IW][C], W f32 [C][N][K][K]), every element drawn from {+-1, +-2, +-3} (never 0: a dropped zero term
    would be invisible).  |Y| <= 9 * C * K*K <= 5184: every partial sum is exact in f32 in ANY order, so Y_nchw has to equal
    the reference bit for bit and Y its nearest-even bf16 rounding."""
    gen = torch.Generator().manual_seed(seed)
    X = _int_tensor((tn.B, tn.IH, tn.IW, tn.C), tn.C, G.BF16, gen)
    W = _VALS[torch.randint(0, 6, (tn.C, tn.N, tn.K, tn.K), generator=gen)]
    return X, W


def tn_eps(tn, seed):
    """Integer "noise" [B][N][OH][OW] f32 in {+-1, +-2, +-3}."""
    gen = torch.Generator().manual_seed(seed)
    return _VALS[torch.randint(0, 6, (tn.B, tn.N, tn.OH, tn.OW), generator=gen)]


def bf16_spacing(x):
    """Distance from bf16(|x|) to the next bf16 above it."""
    b = torch.tensor([abs(float(x))]).to(torch.bfloat16)
    return float((b.view(torch.int16) + 1).view(torch.bfloat16).float() - b.float())


def tn_sigma(ref):
    """A power of two above the bf16 spacing of every value v + sigma*eps can take: bf16 keeps 8 significant bits (spacing
    2^(e - 7) for 2^e <= |v| < 2^(e + 1)); 2^(e - 5) at the binade of the largest |v| is four steps there and still two in the
    next binade, which |v| + 3 sigma cannot leave.  One unit of eps then moves every output by more than its rounding, and
    v + sigma*eps is an exact f32 sum of multiples of sigma."""
    top = float(ref.abs().max())
    sigma = 2.0 ** (math.floor(math.log2(top)) - 5)
    assert sigma > bf16_spacing(top + 3 * sigma) >= bf16_spacing(top)
    return sigma


def ew_operands(ew, seed):
    """-> (wide [B][WH][WW][C], narrow [B][NH][NW][8]) bf16: the real channels from {+-1, +-2, +-3}, channels N..7 of the narrow
    operand 0.  Every partial sum is an integer of magnitude <= 9 M (M wide pixels): below 2^24 exact in f32 in any order; the
    factor 2 covers the accumulating call."""
    M = ew.B * ew.WH * ew.WW
    assert 2 * 9 * M < 2 ** 24, f"M = {M}: integer sums would leave the exact range of f32"
    gen = torch.Generator().manual_seed(seed)
    wide = _int_tensor((ew.B, ew.WH, ew.WW, ew.C), ew.C, G.BF16, gen)
    narrow = _int_tensor((ew.B, ew.NH, ew.NW, 8), ew.N, G.BF16, gen)
    return wide, narrow


def ew_int_dw(ew, seed):
    """A second integer tensor (|x| <= 3) to accumulate onto."""
    gen = torch.Generator().manual_seed(seed)
    return _VALS[torch.randint(0, 6, (ew.C * ew.s_c,), generator=gen)]


# ---- vg_tnconv: the case table ---------------------------------------------------------------------------------------------
TN_PLAN_KEYS = ("nt", "kc", "tc", "ro", "co", "tiles_x", "tiles_y")


@dataclasses.dataclass(frozen=True)
class TnCase:
    C: int
    N: int
    k: int
    s: int
    p: int
    H: int
    B: int
    plan: tuple            # (nt, kc, tc, ro, co, tiles_x, tiles_y) of vg_tnconv_plan without in-kernel noise
    rng_plan: tuple = ()   # the same with in-kernel noise, where the row is run with it (`rng` facets)
    why: tuple = ()        # the facets of the tiling the row is there for (TN_FACETS)

    @property
    def id(self):
        return f"C{self.C}-N{self.N}-k{self.k}s{self.s}p{self.p}-H{self.H}-B{self.B}"

    def spec(self):
        sp = G.tn_spec(self.B, self.H, self.H, self.C, self.N, self.k, self.s, self.p, G.BF16, s_n=self.k * self.k,
                       s_c=self.N * self.k * self.k)
        assert sp is not None, self.id
        return sp


# facet -> what the plan records (without / with in-kernel noise), the spec and the row have to show
TN_FACETS = {
    "c16_k3": lambda c, tn, p, r: tn.C == 16 and tn.K == 3,
    "c16_k4": lambda c, tn, p, r: tn.C == 16 and tn.K == 4,
    "whole_rows_row_tiles": lambda c, tn, p, r: p["tiles_x"] == 1 and p["tc"] == tn.IW and p["tiles_y"] >= 3,
    "blocks_partial_edges": lambda c, tn, p, r: p["tiles_x"] > 1 and tn.OW % p["co"] != 0 and tn.OH % p["ro"] != 0,
    # one tile whose window leaves groups of the LDS tile unused: the last waves own no pixel group at all
    "one_tile_idle_waves": lambda c, tn, p, r: p["grid"] == 1 and tn.IH * tn.IW <= p["npix"] // 2,
    "batch": lambda c, tn, p, r: tn.B > 1 and p["grid"] == tn.B * p["tiles_x"] * p["tiles_y"],
    "p0": lambda c, tn, p, r: tn.P == 0,
    "p2": lambda c, tn, p, r: tn.P == 2,
    "rng_replans": lambda c, tn, p, r: r["quad_noise"] and any(p[k] != r[k] for k in TN_PLAN_KEYS),
    "rng_column_step_4": lambda c, tn, p, r: r["quad_noise"] and r["tiles_x"] > 1 and r["co"] % 4 == 0 and p["co"] % 4 != 0,
    "rng_no_quads": lambda c, tn, p, r: tn.OW % 4 != 0 and not r["quad_noise"],
    "rng_no_quads_blocks": lambda c, tn, p, r: tn.OW % 4 != 0 and not r["quad_noise"] and r["tiles_x"] > 1,
}

TN_CASES = [
    # K = 3 (the Generator's last layer): nt 1..3 x kc 1..2
    TnCase(16, 1, 3, 1, 1, 16, 1, (1, 1, 16, 16, 16, 1, 1), why=("c16_k3", "one_tile_idle_waves")),
    TnCase(64, 1, 3, 1, 0, 16, 2, (1, 2, 16, 18, 18, 1, 1), (1, 2, 16, 18, 18, 1, 1), why=("p0", "batch", "rng_no_quads")),
    TnCase(32, 3, 3, 1, 1, 48, 1, (2, 1, 16, 30, 14, 4, 2), (2, 1, 48, 8, 48, 1, 6), why=("blocks_partial_edges", "rng_replans")),
    TnCase(64, 3, 3, 1, 1, 32, 2, (2, 2, 32, 14, 32, 1, 3), why=("whole_rows_row_tiles", "batch")),
    TnCase(32, 4, 3, 1, 2, 32, 1, (3, 1, 16, 14, 14, 3, 3), (3, 1, 16, 14, 14, 3, 3),
           why=("p2", "blocks_partial_edges", "rng_no_quads_blocks")),
    TnCase(32, 4, 3, 1, 1, 48, 1, (3, 1, 16, 14, 14, 4, 4), (3, 1, 16, 14, 12, 4, 4), why=("rng_replans", "rng_column_step_4")),
    TnCase(64, 4, 3, 1, 1, 32, 1, (3, 2, 16, 14, 14, 3, 3), (3, 2, 32, 6, 32, 1, 6), why=("blocks_partial_edges", "rng_replans")),
    # K = 4 (the image gradient below the Discriminator's first layer): nt 1..4 x kc 1..2
    TnCase(16, 1, 4, 2, 1, 16, 1, (1, 1, 16, 32, 32, 1, 1), why=("c16_k4", "one_tile_idle_waves")),
    TnCase(64, 1, 4, 2, 1, 32, 2, (1, 2, 32, 28, 64, 1, 3), why=("whole_rows_row_tiles", "batch")),
    TnCase(32, 2, 4, 2, 0, 16, 1, (2, 1, 16, 34, 34, 1, 1), (2, 1, 16, 34, 34, 1, 1), why=("p0", "rng_no_quads")),
    TnCase(64, 2, 4, 2, 2, 32, 1, (2, 2, 32, 28, 62, 1, 3), why=("p2", "whole_rows_row_tiles")),
    TnCase(32, 3, 4, 2, 1, 48, 1, (3, 1, 16, 28, 28, 4, 4), why=("blocks_partial_edges",)),
    TnCase(64, 3, 4, 2, 1, 16, 3, (3, 2, 16, 28, 32, 1, 2), why=("batch",)),
    TnCase(32, 4, 4, 2, 1, 16, 1, (4, 1, 16, 28, 32, 1, 2)),
    TnCase(64, 4, 4, 2, 1, 32, 1, (4, 2, 32, 12, 64, 1, 6), why=("whole_rows_row_tiles",)),
]
TN_IDS = [c.id for c in TN_CASES]
TN_RNG_CASES = [c for c in TN_CASES if c.rng_plan]
TN_RNG_IDS = [c.id for c in TN_RNG_CASES]
# every tnconv_kernel<NT, KC, ., K, S> the launcher can instantiate, as (nt, kc, K)
TN_INSTANTIATIONS = {(nt, kc, 3) for nt in (1, 2, 3) for kc in (1, 2)} | {(nt, kc, 4) for nt in (1, 2, 3, 4) for kc in (1, 2)}


def tn_plan_tuple(p):
    return tuple(p[k] for k in TN_PLAN_KEYS)


# ---- vg_edge_wgrad: the case table -----------------------------------------------------------------------------------------
EW_PLAN_KEYS = ("ct", "jt", "rows_per_tile", "ntiles", "grid")


@dataclasses.dataclass(frozen=True)
class EwCase:
    kind: str              # conv: the narrow side is the input of Conv2d(N, C); convT: the output of ConvTranspose2d(C, N)
    C: int
    N: int
    k: int
    s: int
    p: int
    H: int
    B: int
    plan: tuple            # (ct, jt, rows_per_tile, ntiles, grid) of vg_edge_wgrad_plan
    why: tuple = ()        # EW_FACETS

    @property
    def id(self):
        return f"{self.kind}-C{self.C}-N{self.N}-k{self.k}s{self.s}p{self.p}-H{self.H}-B{self.B}"

    def spec(self):
        if self.kind == "conv":
            ew = G.conv_wgrad_edge(self.B, self.H, self.H, self.N, self.C, self.k, self.s, self.p, G.BF16)
        else:
            ew = G.convT_wgrad_edge(self.B, self.H, self.H, self.C, self.N, self.k, self.s, self.p, G.BF16)
        assert ew is not None, self.id
        return ew


def ew_walk(p):
    """Tiles per workgroup of a plan record: workgroup w does tiles w, w + grid, ... -> (most, fewest)."""
    return -(-p["ntiles"] // p["grid"]), p["ntiles"] // p["grid"]


def _short(ew, p):
    return ew.WH % p["rows_per_tile"] != 0


EW_FACETS = {
    "short_last_tile": lambda ew, p: _short(ew, p) and ew_walk(p) == (1, 1),
    "pad_pixels": lambda ew, p: p["rows_per_tile"] * ew.WW < 256 and ew.WH >= p["rows_per_tile"],   # tiles of fewer than 256 pixels
    "walk_2_and_1": lambda ew, p: p["ntiles"] > p["grid"] and ew_walk(p) == (2, 1),
    "walk_3_across_images": lambda ew, p: ew_walk(p) == (3, 2) and p["tiles_per_img"] == 1,     # every step is another image
    "walk_into_next_image": lambda ew, p: p["ntiles"] > p["grid"] and p["rows_per_tile"] == 1 and p["grid"] % p["tiles_per_img"] == 0,
    "walk_with_short_tile": lambda ew, p: _short(ew, p)                                         # a second tile that is a short one
    and any((t + 1) % p["tiles_per_img"] == 0 for t in range(p["grid"], p["ntiles"])),
}

EW_CASES = [
    EwCase("conv", 64, 3, 4, 2, 1, 64, 3, (4, 4, 8, 12, 12)),                                   # Discriminator's first layer at S=64
    EwCase("convT", 64, 3, 3, 1, 1, 64, 2, (4, 3, 4, 32, 32)),                                  # Generator's last layer at S=64
    EwCase("conv", 32, 2, 4, 2, 0, 64, 2, (2, 4, 8, 8, 8), why=("short_last_tile", "pad_pixels")),   # 31 x 31 wide, R 8: 7 rows left
    EwCase("convT", 32, 1, 3, 1, 1, 32, 2, (2, 3, 8, 8, 8)),
    EwCase("conv", 16, 1, 4, 2, 1, 32, 3, (1, 4, 16, 3, 3)),
    EwCase("convT", 16, 2, 3, 1, 1, 48, 1, (1, 3, 5, 10, 10), why=("short_last_tile", "pad_pixels")),   # 5 x 48 = 240 pixels, 3 rows left
    # ntiles > grid: the grid-stride walk, the barrier between tiles and the accumulators that live across them
    EwCase("conv", 64, 3, 4, 2, 1, 64, 130, (4, 4, 8, 520, 512), why=("walk_2_and_1",)),
    EwCase("conv", 32, 2, 4, 2, 0, 64, 130, (2, 4, 8, 520, 512), why=("walk_2_and_1", "walk_with_short_tile")),
    EwCase("conv", 16, 1, 4, 2, 1, 32, 1100, (1, 4, 16, 1100, 512), why=("walk_3_across_images",)),
    EwCase("convT", 16, 3, 3, 1, 1, 256, 3, (1, 3, 1, 768, 512), why=("walk_2_and_1", "walk_into_next_image")),
]
EW_IDS = [c.id for c in EW_CASES]


def ew_plan_tuple(p):
    return tuple(p[k] for k in EW_PLAN_KEYS)
