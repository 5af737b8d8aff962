"""Host plan of tiled denoising (numpy only; importable without a GPU): an H x W image is cut into overlapping S x S tiles,
the tiles go through Encoder -> reparameterise -> Generator in batches, and the reconstructions are blended back with a
separable window.  The plan fixes the tile origins and, per axis and coordinate, the normalised blend coefficients, so the
blend kernel (csrc/tiling.hip, vg_tile_blend) only multiplies and adds: it never divides.

Per axis of length L: origins 0, stride, 2 stride, ... while < L - S, then one last tile flush with the edge at L - S (no
padding: the last tile simply overlaps more); L == S: the single origin 0.  Tile t = ky * nx + kx.  For coordinate p the
covering tiles are a contiguous range first[p] .. first[p] + count[p] - 1, and

    coef[p][j] = w[p - o_k] / sum_k w[p - o_k]        (k = first[p] + j; f64, rounded once to f32; unused slots 0)

The blend (include/vaegan_hip.h "Tiled denoising"; restated in tests/_tiling_ref.py), all arithmetic f32:

    out[n,c,y,x] = sum_{ky ascending} coef_y[y][ky] * ( sum_{kx ascending} coef_x[x][kx] * r[n, ky nx + kx, c, y - oy[ky], x - ox[kx]] )
"""
from typing import Optional

import numpy as np

VG_TILE_MAX_COVER = 8          # include/vaegan_hip.h: most tiles that may cover one coordinate of an axis
WINDOWS = ("box", "tri", "hann")


def window_weights(name: str, S: int) -> np.ndarray:
    """f64 [S], strictly positive (the half-sample offset keeps the ends off zero), symmetric."""
    i = np.arange(S, dtype=np.float64)
    if name == "box":
        return np.ones(S, dtype=np.float64)
    if name == "tri":
        return np.minimum(i + 0.5, S - 0.5 - i) / (S / 2.0)
    if name == "hann":
        return np.sin(np.pi * (i + 0.5) / S) ** 2
    raise RuntimeError(f"tile_plan: unknown window {name!r} (one of {WINDOWS})")


def axis_origins(L: int, S: int, stride: int) -> np.ndarray:
    o = list(range(0, max(L - S, 0), stride)) + [L - S]
    return np.asarray(o, dtype=np.int32)


def axis_tables(L: int, S: int, origins: np.ndarray, w: np.ndarray):
    """-> (first int32 [L], count int32 [L], coef f32 [L][width]) with width = the largest cover count of the axis."""
    o = origins.astype(np.int64)
    p = np.arange(L, dtype=np.int64)
    covers = (o[None, :] <= p[:, None]) & (p[:, None] < o[None, :] + S)              # [L][n]
    count = covers.sum(axis=1)
    first = covers.argmax(axis=1)
    width = int(count.max())
    coef = np.zeros((L, width), dtype=np.float32)
    for q in range(L):
        ws = w[q - o[first[q]:first[q] + count[q]]]
        coef[q, :count[q]] = (ws / ws.sum()).astype(np.float32)
    return first.astype(np.int32), count.astype(np.int32), coef


class TilePlan:
    """Geometry and coefficient tables of one (H, W, S, stride, window).  Host arrays: oy int32 [ny], ox int32 [nx];
    first_y, count_y int32 [H], coef_y f32 [H][cover_y]; the same for x.  ``device_tables(device)`` uploads them once and
    keeps them on the plan (ops.tile_gather / ops.tile_blend)."""

    def __init__(self, H, W, S, stride, window_name, oy, ox, first_y, count_y, coef_y, first_x, count_x, coef_x):
        self.H, self.W, self.S, self.stride, self.window = int(H), int(W), int(S), int(stride), window_name
        self.oy, self.ox = np.ascontiguousarray(oy, dtype=np.int32), np.ascontiguousarray(ox, dtype=np.int32)
        self.first_y, self.count_y = (np.ascontiguousarray(a, dtype=np.int32) for a in (first_y, count_y))
        self.first_x, self.count_x = (np.ascontiguousarray(a, dtype=np.int32) for a in (first_x, count_x))
        self.coef_y, self.coef_x = (np.ascontiguousarray(a, dtype=np.float32) for a in (coef_y, coef_x))
        self.ny, self.nx = int(self.oy.size), int(self.ox.size)
        self.cover_y, self.cover_x = int(self.coef_y.shape[1]), int(self.coef_x.shape[1])
        if self.coef_y.shape[0] != self.H or self.coef_x.shape[0] != self.W or self.first_y.size != self.H or \
                self.count_y.size != self.H or self.first_x.size != self.W or self.count_x.size != self.W:
            raise RuntimeError("TilePlan: the tables do not have one row per coordinate")
        if not (1 <= self.cover_y <= VG_TILE_MAX_COVER and 1 <= self.cover_x <= VG_TILE_MAX_COVER):
            raise RuntimeError(f"TilePlan: a cover count above VG_TILE_MAX_COVER = {VG_TILE_MAX_COVER}")
        self._device = {}

    @property
    def tiles_per_image(self) -> int:
        return self.ny * self.nx

    def device_tables(self, device):
        """The eight tables as device tensors (int32 / f32), uploaded on first use per device."""
        import torch
        key = str(device)
        t = self._device.get(key)
        if t is None:
            t = {k: torch.from_numpy(getattr(self, k)).to(device) for k in
                 ("oy", "ox", "first_y", "count_y", "coef_y", "first_x", "count_x", "coef_x")}
            self._device[key] = t
        return t

    def __repr__(self):
        return (f"TilePlan(H={self.H}, W={self.W}, S={self.S}, stride={self.stride}, window={self.window!r}, "
                f"tiles={self.ny}x{self.nx}, cover={self.cover_y}x{self.cover_x})")


def tile_plan(H: int, W: int, S: int, stride: Optional[int] = None, window: str = "hann") -> TilePlan:
    H, W, S = int(H), int(W), int(S)
    if S < 1 or H < S or W < S:
        raise RuntimeError(f"tile_plan: the image ({H} x {W}) is smaller than the tile ({S} x {S}); there is no padding")
    stride = S // 2 if stride is None else int(stride)
    if stride < 1 or stride > S:
        raise RuntimeError(f"tile_plan: stride {stride} outside [1, {S}] (a stride above the tile size leaves gaps)")
    w = window_weights(window, S)
    oy, ox = axis_origins(H, S, stride), axis_origins(W, S, stride)
    fy, cy, ky = axis_tables(H, S, oy, w)
    fx, cx, kx = axis_tables(W, S, ox, w)
    if max(ky.shape[1], kx.shape[1]) > VG_TILE_MAX_COVER:
        raise RuntimeError(f"tile_plan: stride {stride} lets {max(ky.shape[1], kx.shape[1])} tiles cover one coordinate; "
                           f"at most VG_TILE_MAX_COVER = {VG_TILE_MAX_COVER}")
    return TilePlan(H, W, S, stride, window, oy, ox, fy, cy, ky, fx, cx, kx)


_PLANS = {}


def cached_plan(H: int, W: int, S: int, stride: Optional[int] = None, window: str = "hann") -> TilePlan:
    """tile_plan, remembered per geometry: repeated calls on images of one size reuse the plan and its device tables."""
    key = (int(H), int(W), int(S), None if stride is None else int(stride), window)
    plan = _PLANS.get(key)
    if plan is None:
        plan = _PLANS[key] = tile_plan(H, W, S, stride, window)
    return plan
