"""f64 numpy restatement of the two contracts of include/vaegan_hip.h "Non-local means baseline and blind noise estimate"
(vg_nlm_denoise, vg_noise_sigma), the counted first-order error bound of the NLM kernel, a definition-order form for tiny
cases, and the exact-input table that makes the bitwise GPU cases safe.

The bound.  With u = 2^-24 (unit roundoff of f32) the kernel (csrc/nlm.hip) computes, per pixel p and offset t,

    S    the channel-summed squared differences, box-summed: every term passes one subtraction (u), one squaring inside an
         fma (the product is exact, the fma rounds once: with the subtraction's error doubled, 3u in all), then at most
         (C - 1) further fmas over the channels, 2P adds of the row box sum and 2P adds of the column box sum; all terms are
         >= 0, so relative errors do not grow:                                         |dS|  <= (3 + (C - 1) + 4P) u S
    d2   = S * fl(1/n): the constant's rounding and the product's                      |dd2| <= (C + 4P + 4) u d2
    e    = max(d2 - fl(2 fl(sigma^2)), 0): sigma^2 rounds once (times 2 is exact), the subtraction once on a result of
         size <= d2 + 2 sigma^2; max is 1-Lipschitz                                    |de|  <= (C + 4P + 6) u (d2 + 2 sigma^2)
    arg  = e * nscale, nscale = fl(fl(-log2 e) / fl(h * h)), h = fl(fl(h_factor * sigma) + h_const): h 2u (a fused
         multiply-add gives less), h * h 2 * 2u + u, the constant u, the quotient u, the product u: 8u relative to
         a = e / h^2 <= (d2 + 2 sigma^2) / h^2

so  delta_a_t = c u (d2_t + 2 sigma^2) / h^2  with  c = C + 4P + 14  (NLM_C_CONST).  The hardware exponential v_exp_f32 is
accurate to 1 ulp of its result, eps_exp = 2^-23 = 2u (NLM_EPS_EXP; results below 2^-126 are flushed to 0, an absolute
2^-126 next to a weight sum >= 1 -- the centre -- and far inside the last term).  A weight error delta_w_t = w_t (delta_a_t +
eps_exp) moves the quotient by delta_w_t (x~(p+t) - y(p)) / sum w, and the K-term sums by fma and the one division move it by
at most (K + 3) u max|x| in first order:

    bound(p) = sum_t w_t (delta_a_t + eps_exp) |x~(p+t) - y(p)| / sum_t w_t  +  (K + 3) u max|x|.

The noise estimate is evaluated in f64 on the device (the mask response of nine f32 and the sum of at most 2^31 terms): against
this restatement it differs by the final f32 rounding and a relative (n + 16) 2^-53 of the f64 sum, n the summand count."""
import math

import numpy as np

U = 2.0 ** -24
NLM_EPS_EXP = 2.0 ** -23
MASK = np.array([[1, -2, 1], [-2, 4, -2], [1, -2, 1]], dtype=np.float64)


def nlm_c_const(C, P):
    return C + 4 * P + 14


def image_params(sigma, b, h_factor, h_const):
    """(sigma_b, h_b, pass_through) as the contract states them; h_factor / h_const travel as f32.  The pass-through
    decision is taken on h_b as f32 arithmetic gives it (an overflow to inf passes the image through); the value is f64."""
    s = 0.0 if sigma is None else float(np.float32(sigma[b]))
    h = float(np.float32(h_factor)) * s + float(np.float32(h_const))
    with np.errstate(over="ignore", invalid="ignore"):
        h32 = float(np.float32(h_factor) * np.float32(s) + np.float32(h_const))
    return s, h, not (math.isfinite(h32) and h32 > 0.0 and math.isfinite(s))


def _box(D, P, H, W):
    """[H + 2P, W + 2P] -> [H, W] sums over (2P+1)^2 windows: rows, then columns."""
    r = sum(D[:, k:k + W] for k in range(2 * P + 1))
    return sum(r[k:k + H, :] for k in range(2 * P + 1))


def _offsets(R):
    return [(ty, tx) for ty in range(-R, R + 1) for tx in range(-R, R + 1)]


def patch_d2(xp, P, R, H, W):
    """xp: the reflect-padded image f64 [C, H + 2(P+R), W + 2(P+R)] -> d2 f64 [K, H, W] over the offsets, row-major."""
    C = xp.shape[0]
    n = C * (2 * P + 1) ** 2
    A = xp[:, R:R + H + 2 * P, R:R + W + 2 * P]
    out = np.empty(((2 * R + 1) ** 2, H, W))
    for k, (ty, tx) in enumerate(_offsets(R)):
        Bm = xp[:, R + ty:R + ty + H + 2 * P, R + tx:R + tx + W + 2 * P]
        out[k] = _box(((A - Bm) ** 2).sum(0), P, H, W) / n
    return out


def shifted(xp, P, R, H, W):
    """x~(p + t) f64 [K, C, H, W]."""
    HALO = P + R
    return np.stack([xp[:, HALO + ty:HALO + ty + H, HALO + tx:HALO + tx + W] for ty, tx in _offsets(R)])


def nlm_ref(x, sigma, P, R, h_factor, h_const, want_bound=False):
    """x [B,C,H,W] (any float type; evaluated in f64), sigma [B] or None -> y f64 [B,C,H,W] (a pass-through image is x itself)
    and, with want_bound, the per-element first-order bound of the module docstring (0 for a pass-through image)."""
    x = np.asarray(x)
    B, C, H, W = x.shape
    HALO, K = P + R, (2 * R + 1) ** 2
    assert min(H, W) >= HALO + 1
    y = np.empty(x.shape, dtype=np.float64)
    bound = np.zeros(x.shape, dtype=np.float64)
    c = nlm_c_const(C, P)
    for b in range(B):
        s, h, skip = image_params(sigma, b, h_factor, h_const)
        xb = x[b].astype(np.float64)
        if skip:
            y[b] = xb
            continue
        xp = np.pad(xb, ((0, 0), (HALO, HALO), (HALO, HALO)), mode="reflect")
        d2 = patch_d2(xp, P, R, H, W)                                    # [K,H,W]
        w = np.exp(-np.maximum(d2 - 2 * s * s, 0.0) / (h * h))
        xs = shifted(xp, P, R, H, W)                                     # [K,C,H,W]
        den = w.sum(0)
        y[b] = (w[:, None] * xs).sum(0) / den
        if want_bound:
            dw = w * (c * U * (d2 + 2 * s * s) / (h * h) + NLM_EPS_EXP)
            bound[b] = (dw[:, None] * np.abs(xs - y[b][None])).sum(0) / den + (K + 3) * U * np.abs(xb).max()
    return (y, bound) if want_bound else y


def nlm_naive(x, sigma, P, R, h_factor, h_const):
    """The definition, pixel by pixel and offset by offset (tiny cases only)."""
    x = np.asarray(x, dtype=np.float64)
    B, C, H, W = x.shape

    def refl(g, n):
        g = -g if g < 0 else g
        return 2 * (n - 1) - g if g > n - 1 else g
    y = np.empty_like(x)
    for b in range(B):
        s, h, skip = image_params(sigma, b, h_factor, h_const)
        if skip:
            y[b] = x[b]
            continue
        xt = lambda c, i, j: x[b, c, refl(i, H), refl(j, W)]             # noqa: E731
        for i in range(H):
            for j in range(W):
                num, den = np.zeros(C), 0.0
                for ty in range(-R, R + 1):
                    for tx in range(-R, R + 1):
                        d2 = 0.0
                        for c in range(C):
                            for dy in range(-P, P + 1):
                                for dx in range(-P, P + 1):
                                    d2 += (xt(c, i + dy, j + dx) - xt(c, i + ty + dy, j + tx + dx)) ** 2
                        d2 /= C * (2 * P + 1) ** 2
                        w = math.exp(-max(d2 - 2 * s * s, 0.0) / (h * h))
                        den += w
                        for c in range(C):
                            num[c] += w * xt(c, i + ty, j + tx)
                y[b, :, i, j] = num / den
    return y


# ---- the exact-input table ------------------------------------------------------------------------------------------------
EXACT_HF = 2.0 ** -10          # h_b = 2^-10 (sigma_b + 1): at most 2^-9
EXACT_HC = 2.0 ** -10
EXACT_PR = [(0, 1), (2, 5), (3, 10), (1, 10)]
EXACT_C = [1, 3, 4]
TILE = 16                      # the kernel's output tile edge (csrc/nlm.hip NLM_T)


def exact_shapes(P, R):
    """The minimum image (smaller than one tile), one tile exactly, one tile plus one pixel in each direction, ragged in both."""
    m = P + R + 1
    return [(m, m), (TILE, TILE), (TILE + 1, 2 * TILE + 1), (TILE + 3, 2 * TILE + 5)]


def exact_case(P, R, C, H, W, seed=0):
    """-> x f32 [3,C,H,W] of small integers in [-3, 3], sigma f32 [3].
    image 0  sigma = 0: a pattern of period 2 in y and 2..5 in x per channel with values in [-2, 2], a constant block, a few
             single-pixel defects, the value -3 at the corner (0,0) (nowhere else: that pixel matches only itself) and the value
             3 at (1,0) (its only other copy is its reflection about row 0).
    image 1  sigma = sqrt(0.75 / n), n = C (2P+1)^2, so 2 sigma^2 n = 1.5: patches that differ in ONE unit step (S = 1) still
             weigh exactly 1, S >= 2 weighs 0: a constant image with a +1 defect at the corner and, for narrow windows, sparse
             +-1 defects.
    image 2  sigma = -2: h_b < 0, passed through; random integers."""
    rng = np.random.default_rng(1000 * seed + 97 * P + 13 * R + 7 * C + H * 31 + W)
    x = np.zeros((3, C, H, W), dtype=np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    for c in range(C):
        px = 2 + (c + seed) % 4
        tab = rng.integers(-2, 3, size=(2, px))
        x[0, c] = tab[yy % 2, xx % px]
    bh, bw = max(1, H // 3), max(1, W // 3)
    x[0, :, H - bh:, W - bw:] = 1.0                                       # the constant block
    for _ in range(3):                                                    # single-pixel defects away from rows 0..2
        i, j, c = int(rng.integers(min(3, H - 1), H)), int(rng.integers(0, W)), int(rng.integers(0, C))
        x[0, c, i, j] = 2.0 if x[0, c, i, j] != 2.0 else -2.0
    x[0, :, 0, 0] = -3.0
    x[0, :, 1, 0] = 3.0
    if H < 3:
        x[0, :, 0, 1:] = x[0, :, 1, 1:]                                   # the 2 x 2 image: (0,1) matches (1,1) and nothing else
    x[1] = 2.0
    x[1, 0, 0, 0] = 3.0                                                   # its copies are 2(H-1), 2(W-1) apart: one per patch
    nd = (H * W) // 60 if 2 * (P + R) + 1 <= min(15, H, W) else 0         # wide windows: the corner defect alone, so that
    for _ in range(nd):                                                   # patches with no defect still match all K offsets
        i, j = int(rng.integers(0, H)), int(rng.integers(0, W))
        x[1, int(rng.integers(0, C)), i, j] = 2.0 + float(rng.choice([-1.0, 1.0]))
    x[2] = rng.integers(-3, 4, size=(C, H, W)).astype(np.float32)
    n = C * (2 * P + 1) ** 2
    sigma = np.array([0.0, math.sqrt(0.75 / n), -2.0], dtype=np.float32)
    return x, sigma


def nlm_exact(x, sigma, P, R, h_factor=EXACT_HF, h_const=EXACT_HC):
    """The kernel's result on an exact-table input, bit for bit, with the conditions that make it so ASSERTED on this
    reference alone: every S is an integer, every weight is exactly 1 (d2 <= 2 sigma^2, by a margin no f32 rounding of the
    two sides can cross) or has a >= 128 (exp(-128) = 2.6e-56 is 0 in f32, as is the hardware's 2^(-128 log2 e)), all sums
    stay below 2^24.  -> y f32 [B,C,H,W], info: per image the match counts [H,W] (None for a pass-through image) and
    ``only_reflect`` [H,W] bool: the pixel has matches besides itself and every one of them lies outside the image."""
    x = np.asarray(x, dtype=np.float32)
    B, C, H, W = x.shape
    HALO, K = P + R, (2 * R + 1) ** 2
    n = C * (2 * P + 1) ** 2
    assert np.all(x == np.rint(x)) and np.abs(x).max() <= 3
    y = np.empty_like(x)
    counts, only_reflect, soft = [], [], []
    offs = _offsets(R)
    for b in range(B):
        s, h, skip = image_params(sigma, b, h_factor, h_const)
        if skip:
            y[b] = x[b]
            counts.append(None), only_reflect.append(None), soft.append(0)
            continue
        xp = np.pad(x[b].astype(np.float64), ((0, 0), (HALO, HALO), (HALO, HALO)), mode="reflect")
        Sn = patch_d2(xp, P, R, H, W) * n
        S = np.rint(Sn)                                                   # integers
        assert np.abs(Sn - S).max() < 1e-9 and S.max() * 1.0 < 2 ** 24
        thr = 2 * s * s * n                                               # S <= thr: weight 1
        match = S <= thr
        assert not np.any(np.abs(S - thr) < 1e-3 * max(thr, 1.0)) or thr == 0.0, "a patch distance sits on the threshold"
        if thr == 0.0:
            match = S == 0
        miss = ~match
        if miss.any():
            a_min = ((S[miss] - thr) / n).min() / (h * h)
            assert a_min >= 128.0, f"smallest surviving a = {a_min}"
        xs = shifted(xp, P, R, H, W)
        den = match.sum(0).astype(np.float64)
        num = (match[:, None] * xs).sum(0)
        assert np.abs(num).max() < 2 ** 24 and den.max() <= K and den.min() >= 1
        y[b] = np.float32(num) / np.float32(den)[None]                    # one correctly rounded f32 division of exact operands
        counts.append(den.astype(np.int64))
        inside = np.zeros((K, H, W), dtype=bool)
        ii, jj = np.mgrid[0:H, 0:W]
        for k, (ty, tx) in enumerate(offs):
            inside[k] = (ii + ty >= 0) & (ii + ty < H) & (jj + tx >= 0) & (jj + tx < W)
        centre = np.zeros(K, dtype=bool)
        centre[K // 2] = True
        other = match & ~centre[:, None, None]
        only_reflect.append(other.any(0) & ~(other & inside).any(0))
        soft.append(int((match & (S > 0)).sum()))
    return y, {"counts": counts, "only_reflect": only_reflect, "soft_matches": soft, "K": K}


# ---- Immerkaer's estimate -------------------------------------------------------------------------------------------------
def noise_k(C, H, W):
    return math.sqrt(math.pi / 2.0) / (6.0 * C * (H - 2) * (W - 2))


def mask_response(x):
    """[..., H, W] -> the valid 3 x 3 correlation with MASK (symmetric: correlation = convolution), f64 [..., H-2, W-2]."""
    x = np.asarray(x, dtype=np.float64)
    H, W = x.shape[-2:]
    return sum(MASK[a, b] * x[..., a:a + H - 2, b:b + W - 2] for a in range(3) for b in range(3))


def noise_sigma_ref(x):
    """x [B,C,H,W] -> (sigma f32 [B] = (float)(S * k), S f64 [B])."""
    x = np.asarray(x)
    B, C, H, W = x.shape
    S = np.abs(mask_response(x)).reshape(B, -1).sum(1)
    return (S * noise_k(C, H, W)).astype(np.float32), S


# ---- a synthetic test image -------------------------------------------------------------------------------------------------
def synthetic(H=64, W=64):
    """Three channels in [-1, 1]: a sinusoid, a disc, a ramp."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    a = 0.8 * np.sin(2 * np.pi * (xx / 16.0 + yy / 23.0))
    b = np.where((yy - H / 2) ** 2 + (xx - W / 2) ** 2 < (min(H, W) / 4) ** 2, 0.7, -0.6)
    c = (xx + yy) / (H + W - 2) * 1.6 - 0.8
    return np.stack([a, b, c])[None]


def psnr(a, b):
    mse01 = float(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)) / 4.0
    return float("inf") if mse01 == 0 else 10.0 * math.log10(1.0 / mse01)
