"""f64 numpy restatement of the spectral generation metric (include/vaegan_hip.h, "Spectral generation metric"; spectrum.py,
metrics.SpectrumStats / spectral_distance): the yardstick of tests/test_spectrum_cpu.py and tests/test_gpu_spectrum.py.
Nothing here calls the package or shares code with spectrum.py.

  profiles_fft      the metric as a user would write it: np.fft.rfft2 of the centred, windowed image, |.|^2 summed over the
                    channels, Hermitian-half weight, radial bins from an integer loop of its own, the profile by a plain loop
                    in CSR order
  profiles_generic  the kernel's contract for ARBITRARY tables: two matrix products, the squared modulus, the CSR bin sum with
                    the table-safety rules; in f64, or (exact=True) in integers for integer images and tables, where every
                    intermediate is checked to stay below 2^53 so that f64 arithmetic of any order gives the same bits
Also the input generators and the counted error bound of the random-image tests, so that the CPU tests exercise them too."""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53                      # unit roundoff of f64
R_MAX = math.sqrt(0.5)
LIMIT = 2.0 ** 53


# ---- the pieces of the definition --------------------------------------------------------------------------------------
def contract_mean(plane):
    """The mean of one plane in the contract's order: partial[t] = sum of plane[i], i = t, t + 256, ... ascending; then
    partial[t] += partial[t + s] for s = 128 .. 1; one division by H W."""
    flat = np.asarray(plane, np.float64).reshape(-1)
    n = flat.size
    pad = np.zeros((n + 255) // 256 * 256)
    pad[:n] = flat                                   # adding +0.0 changes no partial sum
    part = np.zeros(256)
    for row in pad.reshape(-1, 256):
        part = part + row
    s = 128
    while s:
        part[:s] = part[:s] + part[s:2 * s]
        s //= 2
    return part[0] / float(n)


def hann(N):
    """The periodic Hann window, straight from its formula."""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)


def window(N, kind):
    return hann(N) if kind == "hann" else np.ones(N)


def half_weight(H, W):
    wt = np.empty((H, W // 2 + 1))
    for v in range(W // 2 + 1):
        wt[:, v] = 1.0 if v == 0 or 2 * v == W else 2.0
    return wt


def radial_bin(H, W, n_bins, u, v):
    """The bin of one point by the integer rule: the largest k with k^2 H^2 W^2 <= 2 n_bins^2 (a^2 W^2 + b^2 H^2)."""
    a, b = min(u, H - u), v
    num, den = 2 * n_bins * n_bins * (a * a * W * W + b * b * H * H), H * H * W * W
    k = math.isqrt(num // den)
    assert k * k * den <= num < (k + 1) * (k + 1) * den
    return min(n_bins - 1, k)


def radial_bin_fraction(H, W, n_bins, u, v):
    """The bin of one point by the DEFINITION, k = min(n_bins - 1, floor(n_bins r / r_max)), r^2 = (a/H)^2 + (b/W)^2,
    r_max^2 = 1/2, in Fractions: floor(sqrt(t)) of the exact t = (n_bins r / r_max)^2, found from a float estimate and
    corrected by exact comparisons."""
    a, b = min(u, H - u), v
    t = n_bins * n_bins * (Fraction(a, H) ** 2 + Fraction(b, W) ** 2) / Fraction(1, 2)
    k = int(math.sqrt(float(t)))
    while Fraction(k * k) > t:
        k -= 1
    while Fraction((k + 1) * (k + 1)) <= t:
        k += 1
    return min(n_bins - 1, k)


def radial_csr(H, W, n_bins):
    """(order int32, bin_start int32 [n_bins + 1], counts): every point of the half spectrum, ascending flat index in a bin."""
    Wh = W // 2 + 1
    members = [[] for _ in range(n_bins)]
    for u in range(H):
        for v in range(Wh):
            members[radial_bin(H, W, n_bins, u, v)].append(u * Wh + v)
    order = np.array([o for m in members for o in m], np.int32)
    counts = np.array([len(m) for m in members], np.int64)
    return order, np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), counts


def identity_csr(H, W):
    n = H * (W // 2 + 1)
    return np.arange(n, dtype=np.int32), np.arange(n + 1, dtype=np.int32), np.ones(n, np.int64)


def default_bins(H, W):
    return min(H, W) // 2


def bin_sum(P, weight, order, bin_start, n_bins, HWh):
    """prof[.., k] by a plain loop in ascending j, with the contract's table safety: nnz = bin_start[n_bins] clamped into
    [0, H Wh]; a bin whose bounds are not 0 <= s <= e <= nnz gives 0; an entry outside [0, H Wh) is skipped.  P [.., H Wh]
    (f64 or Python ints as objects); the loop runs over the entries, vectorised over the leading axes only."""
    P = np.asarray(P)
    w = np.asarray(weight).reshape(-1)
    lead = P.shape[:-1]
    prof = np.zeros(lead + (n_bins,), dtype=P.dtype)
    nnz = min(max(int(bin_start[n_bins]), 0), HWh)
    for k in range(n_bins):
        s, e = int(bin_start[k]), int(bin_start[k + 1])
        if s < 0 or e < s or e > nnz:
            continue
        acc = np.zeros(lead, dtype=P.dtype)
        for j in range(s, e):
            o = int(order[j])
            if 0 <= o < HWh:
                acc = acc + w[o] * P[..., o]
        prof[..., k] = acc
    return prof


# ---- restatement 1: the FFT --------------------------------------------------------------------------------------------
def power_fft(x, win="hann", center=True):
    """P [B][H][Wh]: sum over the channels of |rfft2((x - mean) w_H w_W)|^2."""
    x = np.asarray(x, np.float64)
    B, C, H, W = x.shape
    w2 = window(H, win)[:, None] * window(W, win)[None, :]
    P = np.zeros((B, H, W // 2 + 1))
    for b in range(B):
        for c in range(C):
            m = contract_mean(x[b, c]) if center else 0.0
            F = np.fft.rfft2((x[b, c] - m) * w2)
            P[b] += F.real ** 2 + F.imag ** 2
    return P


def profiles_fft(x, n_bins=None, win="hann", center=True, bins="radial"):
    """-> (prof f64 [B][n_bins], P f64 [B][H][Wh])."""
    B, C, H, W = np.asarray(x).shape
    HWh = H * (W // 2 + 1)
    if bins == "2d":
        order, start, _ = identity_csr(H, W)
        n_bins = HWh
    else:
        n_bins = default_bins(H, W) if n_bins is None else n_bins
        order, start, _ = radial_csr(H, W, n_bins)
    P = power_fft(x, win, center)
    return bin_sum(P.reshape(B, HWh), half_weight(H, W), order, start, n_bins, HWh), P


def dft_tables(H, W, win="hann"):
    """The windowed DFT matrices straight from np.exp (no argument reduction): (tw_re, tw_im [W][Wh], th_re, th_im [H][H])."""
    Wh = W // 2 + 1
    tw = window(W, win)[:, None] * np.exp(-2j * np.pi * np.outer(np.arange(W), np.arange(Wh)) / W)
    th = window(H, win)[None, :] * np.exp(-2j * np.pi * np.outer(np.arange(H), np.arange(H)) / H)
    return tw.real.copy(), tw.imag.copy(), th.real.copy(), th.imag.copy()


# ---- restatement 2: arbitrary tables -----------------------------------------------------------------------------------
def profiles_generic(x, center, tw_re, tw_im, th_re, th_im, weight, order, bin_start, n_bins, exact=False):
    """The kernel's contract on the caller's tables -> (prof [B][n_bins], P [B][H][Wh]) in f64.

    exact=True: x and every table hold integers (x may be centred onto multiples of 1/4, see ``exact_images``).  Everything
    is scaled to integers (x - m by 4, so P and prof by 16), evaluated in int64, and every partial sum any summation order
    can meet -- bounded by the sums of absolute values -- is asserted below 2^53 (times the scale): f64 arithmetic is then
    exact in every order, fused or not, and the f64 results returned are THE answer, bit for bit."""
    x = np.asarray(x, np.float64)
    B, C, H, W = x.shape
    Wh = W // 2 + 1
    HWh = H * Wh
    if not exact:
        P = np.zeros((B, H, Wh))
        for b in range(B):
            for c in range(C):
                m = contract_mean(x[b, c]) if center else 0.0
                xc = x[b, c] - m
                yr, yi = xc @ tw_re, xc @ tw_im
                zr = th_re @ yr - th_im @ yi
                zi = th_re @ yi + th_im @ yr
                P[b] += zr * zr + zi * zi
        return bin_sum(P.reshape(B, HWh), weight, order, bin_start, n_bins, HWh), P
    tabs = [np.asarray(t) for t in (tw_re, tw_im, th_re, th_im, weight)]
    assert all((t == np.rint(t)).all() for t in tabs), "exact mode needs integer tables"
    twr, twi, thr, thi, wt = (np.rint(t).astype(np.int64) for t in tabs)
    P = np.zeros((B, H, Wh), np.int64)
    for b in range(B):
        for c in range(C):
            m = contract_mean(x[b, c]) if center else 0.0
            xs = 4.0 * (x[b, c] - m)
            assert (xs == np.rint(xs)).all() and 4.0 * m == np.rint(4.0 * m), "exact mode: x - mean must be a multiple of 1/4"
            xs = np.rint(xs).astype(np.int64)
            yr, yi = xs @ twr, xs @ twi
            zr = thr @ yr - thi @ yi
            zi = thr @ yi + thi @ yr
            P[b] += zr * zr + zi * zi
            ax = np.abs(xs).astype(np.float64)
            ay = np.maximum(ax @ np.abs(twr), ax @ np.abs(twi))                       # bounds every partial sum of stage 1
            az = (np.abs(thr) + np.abs(thi)).astype(np.float64) @ ay                  # ... and of the four products of stage 2
            assert ay.max() < LIMIT and az.max() < LIMIT and 2.0 * C * (az.max() ** 2) < LIMIT, "stage sums reach 2^53"
    assert float(P.max()) < LIMIT
    aw = np.abs(wt).reshape(-1).astype(np.float64)
    assert (P.reshape(B, HWh).astype(np.float64) @ aw).max() < LIMIT, "a bin sum can reach 2^53"
    prof = bin_sum(P.reshape(B, HWh), wt, order, bin_start, n_bins, HWh)
    return prof.astype(np.float64) / 16.0, P.astype(np.float64) / 16.0               # exact: integers below 2^53, a power of 2


def exact_images(B, C, H, W, seed, lo=-3, hi=3, center=True):
    """Integer images in [lo, hi] as f32.  With center, every plane is nudged (pixels raised or lowered inside the range, in
    index order) until its sum is H W / 4 (H W a power of two: the mean is the exact dyadic 1/4) or H W (mean exactly 1; needs
    hi >= 2): a mean that is not zero, so that a kernel that forgets to subtract it is found out, and x - mean a multiple of 1/4."""
    g = np.random.default_rng(seed)
    x = g.integers(lo, hi + 1, size=(B, C, H, W)).astype(np.int64)
    if center:
        n = H * W
        target = n // 4 if n & (n - 1) == 0 else n
        assert target <= hi * n
        for plane in x.reshape(B * C, n):
            d = target - int(plane.sum())
            i = 0
            while d:
                step = min(hi - int(plane[i]), d) if d > 0 else max(lo - int(plane[i]), d)
                plane[i] += step
                d -= step
                i += 1
    return x.astype(np.float32)


def exact_tables(H, W, seed, lo=-2, hi=2):
    """Random integer transform tables and weight in [lo, hi]: (tw_re, tw_im, th_re, th_im, weight) as f64.  No weight is
    0, so that every entry of a bin counts (an entry moved to another bin then shows)."""
    g = np.random.default_rng(seed)
    Wh = W // 2 + 1
    tabs = [g.integers(lo, hi + 1, size=s).astype(np.float64) for s in ((W, Wh), (W, Wh), (H, H), (H, H), (H, Wh))]
    tabs[4] = np.where(tabs[4] == 0, float(hi), tabs[4])
    return tuple(tabs)


EXACT_SHAPES = ((5, 7), (16, 16), (17, 16), (33, 17), (64, 64), (65, 65), (64, 96))
BIN_KINDS = ("one", "two", "default", "identity")


def csr_of_kind(H, W, kind):
    """(order, bin_start, n_bins) of one of the four bin tables every exact shape is run with."""
    if kind == "identity":
        order, start, _ = identity_csr(H, W)
        return order, start, H * (W // 2 + 1)
    n_bins = {"one": 1, "two": 2, "default": default_bins(H, W)}[kind]
    order, start, _ = radial_csr(H, W, n_bins)
    return order, start, n_bins


def exact_case(H, W, B, C, center, seed):
    """(x f32 [B,C,H,W], tables) of one exact row: images in [-3, 3] and tables in [-2, 2]; at 256 x 256 images in [-1, 1],
    tables in {-1, 0, 1} and no centring (the squares would pass 2^53)."""
    big = max(H, W) > 128
    x = exact_images(B, C, H, W, seed, *((-1, 1) if big else (-3, 3)), center=center)
    return x, exact_tables(H, W, seed + 1, *((-1, 1) if big else (-2, 2)))


def mutations(tabs, order, bin_start, n_bins):
    """The blind spots an exact case must see: name -> (tables, bin_start) with one thing wrong."""
    twr, twi, thr, thi, wt = tabs
    shifted = np.array(bin_start).copy()
    if n_bins == 1:
        shifted[1] -= 1
    else:
        shifted[1:n_bins] -= 1                                     # every inner boundary one entry early
    return {"th re/im swapped": ((twr, twi, thi, thr, wt), bin_start),
            "tw re/im swapped with th kept": ((twi, twr, thr, thi, wt), bin_start),
            "th transposed": ((twr, twi, thr.T.copy(), thi.T.copy(), wt), bin_start),
            "weight dropped": ((twr, twi, thr, thi, np.ones_like(wt)), bin_start),
            "bins off by one": ((twr, twi, thr, thi, wt), shifted)}


# ---- the counted bound of the random-image tests -----------------------------------------------------------------------
def profile_bound(x, center, tw_re, tw_im, th_re, th_im, weight, order, bin_start, n_bins):
    """First-order bound on |prof_a - prof_b| for two f64 evaluations of the contract (any summation order inside a
    product), counted, not fitted:
      stage 1: a sum of W products of (x - m), one rounding for the subtraction: |dY| <= (W + 1) u sum|a b|
      stage 2: each part of Z is two sums of H products: |dZ| <= (2 H + 1) u sum|a b|, plus |th| |dY| carried through
      |Z|^2:   d(Z_re^2 + Z_im^2) <= 2 |Z_re| dZ_re + 2 |Z_im| dZ_im, summed over the channels
      bins:    sum |weight| dP over the bin's entries
    and the whole doubled, because both sides are f64 arithmetic of this class."""
    x = np.asarray(x, np.float64)
    B, C, H, W = x.shape
    Wh = W // 2 + 1
    HWh = H * Wh
    atr, ati, ahr, ahi = (np.abs(t) for t in (tw_re, tw_im, th_re, th_im))
    dP = np.zeros((B, H, Wh))
    for b in range(B):
        for c in range(C):
            m = contract_mean(x[b, c]) if center else 0.0
            xc = x[b, c] - m
            ax = np.abs(xc)
            yr, yi = xc @ tw_re, xc @ tw_im
            dyr, dyi = (W + 1) * U * (ax @ atr), (W + 1) * U * (ax @ ati)
            zr = th_re @ yr - th_im @ yi
            zi = th_re @ yi + th_im @ yr
            dzr = (2 * H + 1) * U * (ahr @ np.abs(yr) + ahi @ np.abs(yi)) + ahr @ dyr + ahi @ dyi
            dzi = (2 * H + 1) * U * (ahr @ np.abs(yi) + ahi @ np.abs(yr)) + ahr @ dyi + ahi @ dyr
            dP[b] += 2.0 * np.abs(zr) * dzr + 2.0 * np.abs(zi) * dzi
    return 2.0 * bin_sum(dP.reshape(B, HWh), np.abs(weight), order, bin_start, n_bins, HWh), 2.0 * dP


# ---- the running statistics and the distance ---------------------------------------------------------------------------
def accum(prof, s, q):
    """sum and sumsq after vg_spectrum_accum: one running value per bin, rows added in ascending b."""
    s, q = np.array(s, np.float64), np.array(q, np.float64)
    for row in np.asarray(prof, np.float64):
        s = s + row
        q = q + row * row
    return s, q


def spectral_distance(mean_real, mean_fake, counts, frac_lo, skip_bins=1, hf_from=0.5):
    """dict(lsd_db, hf_share_real, hf_share_fake, hf_excess_db, bins_used, bins_skipped), by loops."""
    d2, used, skipped = 0.0, 0, 0
    tot, hf = [0.0, 0.0], [0.0, 0.0]
    for k in range(len(mean_real)):
        if k < skip_bins or counts[k] == 0:
            continue
        for side, m in enumerate((mean_real, mean_fake)):
            tot[side] += m[k]
            if frac_lo[k] >= hf_from:
                hf[side] += m[k]
        if mean_real[k] > 0 and mean_fake[k] > 0:
            d2 += (10.0 * math.log10(mean_real[k] / mean_fake[k])) ** 2
            used += 1
        else:
            skipped += 1
    sr, sf = hf[0] / tot[0], hf[1] / tot[1]
    return {"lsd_db": math.sqrt(d2 / used) if used else float("nan"), "hf_share_real": sr, "hf_share_fake": sf,
            "hf_excess_db": 10.0 * math.log10(sf / sr) if sr > 0 and sf > 0 else float("nan"), "bins_used": used,
            "bins_skipped": skipped}


# ---- image sets of the detection tests ---------------------------------------------------------------------------------
def smooth_images(n, S, seed, C=1):
    """Gaussian-filtered noise (sigma = 1 px, periodic, applied in the Fourier domain) plus 5 % white noise, each image
    normalised to zero mean and unit standard deviation."""
    g = np.random.default_rng(seed)
    f = np.fft.fftfreq(S)
    gauss = np.exp(-2.0 * (np.pi ** 2) * (f[:, None] ** 2 + f[None, :] ** 2))          # the transform of a sigma = 1 Gaussian
    base = np.fft.ifft2(np.fft.fft2(g.standard_normal((n, C, S, S))) * gauss).real
    base /= base.std(axis=(2, 3), keepdims=True)
    img = base + 0.05 * g.standard_normal((n, C, S, S))
    img -= img.mean(axis=(2, 3), keepdims=True)
    img /= img.std(axis=(2, 3), keepdims=True)
    return img.astype(np.float32)


def checkerboard(S, amp=0.02):
    yy, xx = np.mgrid[0:S, 0:S]
    return (amp * (1.0 - 2.0 * ((yy + xx) & 1))).astype(np.float32)
