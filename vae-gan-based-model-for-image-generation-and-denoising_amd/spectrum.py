"""Host plan of the spectral generation metric: the tables ``vg_spectrum_profiles`` (include/vaegan_hip.h, "Spectral
generation metric") transforms and bins with.

The kernel is a generic separable complex transform followed by a table-driven bin sum; everything that makes it a
windowed 2-D DFT with radial bins is built HERE, in numpy f64 on the host, once per image size:

    tw[x][v] = w_W[x] exp(-2 pi i x v / W)   [W][Wh], Wh = W // 2 + 1 (the Hermitian half of a real image's spectrum)
    th[u][y] = w_H[y] exp(-2 pi i u y / H)   [H][H]
    weight   = 1 for v = 0 and, W even, v = W / 2; 2 elsewhere (the half stands for the whole: the weights sum to H W)
    bins     = "radial": with a = min(u, H - u), b = v, r^2 = (a / H)^2 + (b / W)^2 and r_max^2 = 1 / 2 (the Nyquist corner),
               k = min(n_bins - 1, floor(n_bins r / r_max)), evaluated in exact integers as the largest k with
               k^2 H^2 W^2 <= 2 n_bins^2 (a^2 W^2 + b^2 H^2).  Nothing is dropped: the corner, where the checkerboard of an
               up-convolution lives, falls in the last bin.
               "2d": the identity table, n_bins = H Wh: the mean 2-D spectrum, where up-convolution peaks show as points.

w is the periodic Hann window 0.5 - 0.5 cos(2 pi n / N) (``window="hann"``) or all ones (``"none"``).  The twiddles are
evaluated with the argument reduced in integers first -- x v mod N, then to the first half-quadrant -- so the tables have
the DFT's symmetries exactly (cos and sin of mirrored arguments are the same bits, the quarter points are exactly 0 and 1).
"""
from typing import Dict, Optional

import numpy as np
import torch

MAX_SIZE = 256
WINDOWS = ("hann", "none")
BINS = ("radial", "2d")
R_MAX = float(np.sqrt(0.5))


def _cos_sin(n: np.ndarray, N: int):
    """cos(2 pi n / N), sin(2 pi n / N) for integer n, exactly symmetric: the angle is (pi / 2) (4 n mod 4 N) / N = a quarter
    turn count k plus (pi / 2) rho / N with 0 <= rho < N; rho past the middle of the quadrant is mirrored, so cos and sin
    are only ever evaluated on [0, pi / 4]."""
    a = (4 * (np.asarray(n, dtype=np.int64) % N)) % (4 * N)
    k, rho = a // N, a % N
    mirror = 2 * rho > N
    t = np.where(mirror, N - rho, rho).astype(np.float64)
    c0, s0 = np.cos(np.pi * t / (2.0 * N)), np.sin(np.pi * t / (2.0 * N))
    middle = 2 * rho == N                                              # pi / 4: cos and sin are ONE number
    c0, s0 = np.where(middle, np.sqrt(0.5), c0), np.where(middle, np.sqrt(0.5), s0)
    c, s = np.where(mirror, s0, c0), np.where(mirror, c0, s0)          # inside the quadrant
    cos = np.select([k == 0, k == 1, k == 2], [c, -s, -c], s)
    sin = np.select([k == 0, k == 1, k == 2], [s, c, -s], -c)
    return cos + 0.0, sin + 0.0                                        # + 0.0: no negative zeros in the tables


def window_table(N: int, window: str) -> np.ndarray:
    if window == "none":
        return np.ones(N, dtype=np.float64)
    return 0.5 - 0.5 * _cos_sin(np.arange(N), N)[0]


def dft_table(N: int, n_out: int, window: str, window_on_rows: bool):
    """(re, im) of w exp(-2 pi i j k / N): [N][n_out] with the window on the row index (tw) or [n_out][N] with the window on
    the column index (th, n_out = N)."""
    w = window_table(N, window)
    if window_on_rows:
        jk = np.outer(np.arange(N, dtype=np.int64), np.arange(n_out, dtype=np.int64))
        w = w[:, None]
    else:
        jk = np.outer(np.arange(n_out, dtype=np.int64), np.arange(N, dtype=np.int64))
        w = w[None, :]
    c, s = _cos_sin(jk, N)
    return np.ascontiguousarray(w * c), np.ascontiguousarray(w * -s + 0.0)


def half_weight(H: int, W: int) -> np.ndarray:
    Wh = W // 2 + 1
    wt = np.full((H, Wh), 2.0)
    wt[:, 0] = 1.0
    if W % 2 == 0:
        wt[:, W // 2] = 1.0
    return wt


def radial_bins(H: int, W: int, n_bins: int) -> np.ndarray:
    """int64 [H][Wh]: the bin of every point of the half spectrum, in exact integer arithmetic (all terms below 2^49)."""
    Wh = W // 2 + 1
    u = np.arange(H, dtype=np.int64)
    a = np.minimum(u, H - u)[:, None]
    b = np.arange(Wh, dtype=np.int64)[None, :]
    num = 2 * n_bins * n_bins * (a * a * W * W + b * b * H * H)
    q = num // (H * H * W * W)                       # k^2 <= num / den  <=>  k^2 <= floor(num / den)
    k = np.floor(np.sqrt(q.astype(np.float64))).astype(np.int64)
    k = np.where(k * k > q, k - 1, k)
    k = np.where((k + 1) * (k + 1) <= q, k + 1, k)
    return np.minimum(k, n_bins - 1)


class SpectrumPlan:
    """The tables of one image size (numpy f64 / int32, C-contiguous), bin centres in cycles per pixel and bin counts;
    ``device_tables(device)`` uploads them once per device and caches the copies."""

    def __init__(self, H: int, W: int, n_bins: Optional[int], window: str, bins: str):
        for name, val in (("H", H), ("W", W)):
            if isinstance(val, bool) or not isinstance(val, (int, np.integer)) or not 2 <= val <= MAX_SIZE:
                raise RuntimeError(f"spectrum_plan: {name} must be an integer in [2, {MAX_SIZE}], got {val!r}")
        if window not in WINDOWS:
            raise RuntimeError(f"spectrum_plan: window must be one of {WINDOWS}, got {window!r}")
        if bins not in BINS:
            raise RuntimeError(f"spectrum_plan: bins must be one of {BINS}, got {bins!r}")
        H, W = int(H), int(W)
        Wh = W // 2 + 1
        if n_bins is not None and (isinstance(n_bins, bool) or not isinstance(n_bins, (int, np.integer))):
            raise RuntimeError(f"spectrum_plan: n_bins must be an integer or None, got {n_bins!r}")
        if bins == "radial":
            n_bins = min(H, W) // 2 if n_bins is None else int(n_bins)
            if not 1 <= n_bins <= min(H, W):
                raise RuntimeError(f"spectrum_plan: n_bins must be in [1, min(H, W) = {min(H, W)}], got {n_bins}")
        else:
            if n_bins is not None and int(n_bins) != H * Wh:
                raise RuntimeError(f"spectrum_plan: bins='2d' has n_bins = H * (W // 2 + 1) = {H * Wh}, got {n_bins}")
            n_bins = H * Wh
        self.H, self.W, self.Wh, self.n_bins, self.window, self.bins = H, W, Wh, n_bins, window, bins
        self.tw_re, self.tw_im = dft_table(W, Wh, window, True)
        self.th_re, self.th_im = dft_table(H, H, window, False)
        self.weight = half_weight(H, W)
        u = np.arange(H)
        a, b = np.minimum(u, H - u)[:, None], np.arange(Wh)[None, :]
        radius = np.sqrt((a / H) ** 2 + (b / W) ** 2)                      # cycles per pixel
        if bins == "radial":
            self.bin_of = radial_bins(H, W, n_bins)
            flat = self.bin_of.reshape(-1)
            self.order = np.argsort(flat, kind="stable").astype(np.int32)  # ascending flat index inside a bin
            self.counts = np.bincount(flat, minlength=n_bins).astype(np.int64)
            self.centers = (np.arange(n_bins) + 0.5) / n_bins * R_MAX
            self.frac_lo = np.arange(n_bins) / n_bins                      # a bin's lower edge as a fraction of r_max
        else:
            self.bin_of = np.arange(H * Wh, dtype=np.int64).reshape(H, Wh)
            self.order = np.arange(H * Wh, dtype=np.int32)
            self.counts = np.ones(H * Wh, dtype=np.int64)
            self.centers = radius.reshape(-1).copy()
            self.frac_lo = self.centers / R_MAX
        self.bin_start = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int32)
        self._device: Dict[str, Dict[str, torch.Tensor]] = {}

    TABLES = ("tw_re", "tw_im", "th_re", "th_im", "weight", "order", "bin_start")

    def device_tables(self, device) -> Dict[str, torch.Tensor]:
        key = str(torch.device(device))
        if key not in self._device:
            self._device[key] = {n: torch.from_numpy(np.ascontiguousarray(getattr(self, n))).to(device) for n in self.TABLES}
        return self._device[key]

    def same_bins(self, other: "SpectrumPlan") -> bool:
        return (self.H, self.W, self.n_bins, self.window, self.bins) == (other.H, other.W, other.n_bins, other.window,
                                                                         other.bins)

    def flops(self, C: int) -> float:
        """f64 FLOPs of the two products per image: 2 C H W Wh (2 + 4 H / W)."""
        return 2.0 * C * self.H * self.W * self.Wh * (2.0 + 4.0 * self.H / self.W)

    def __repr__(self):
        return f"SpectrumPlan(H={self.H}, W={self.W}, n_bins={self.n_bins}, window={self.window!r}, bins={self.bins!r})"


def spectrum_plan(H: int, W: int, n_bins: Optional[int] = None, window: str = "hann", bins: str = "radial") -> SpectrumPlan:
    """The plan of H x W images: ``n_bins`` radial bins (default min(H, W) // 2, at most min(H, W)) or, ``bins="2d"``, the
    identity table of the mean 2-D spectrum."""
    return SpectrumPlan(H, W, n_bins, window, bins)
