"""numpy restatement of tiled denoising, written from include/vaegan_hip.h ("Tiled denoising") and the issue's contract, not
from tiling.py or csrc/tiling.hip: the plan (origins, cover ranges, normalised coefficients), the gather from both sources,
and the blend in the contract's order in f32, plus an f64 form that divides by the summed window instead of using the
rounded coefficients."""
from types import SimpleNamespace

import numpy as np

MAX_COVER = 8
f32 = np.float32


def window(name, S):
    i = np.arange(S, dtype=np.float64)
    if name == "box":
        return np.ones(S)
    if name == "tri":
        return np.minimum(i + 0.5, S - 0.5 - i) / (S / 2.0)
    if name == "hann":
        return np.sin(np.pi * (i + 0.5) / S) ** 2
    raise ValueError(name)


def origins(L, S, stride):
    o, k = [], 0
    while k * stride < L - S:
        o.append(k * stride)
        k += 1
    o.append(L - S)
    return o


def axis(L, S, stride, w):
    """-> (origins, first [L], count [L], coef f32 [L][width])"""
    o = origins(L, S, stride)
    cover = [[k for k, ok in enumerate(o) if ok <= p < ok + S] for p in range(L)]
    for ks in cover:
        assert ks and ks == list(range(ks[0], ks[0] + len(ks)))            # never empty, always contiguous
    width = max(len(ks) for ks in cover)
    coef = np.zeros((L, width), dtype=np.float32)
    for p, ks in enumerate(cover):
        ws = np.array([w[p - o[k]] for k in ks], dtype=np.float64)
        coef[p, :len(ks)] = (ws / ws.sum()).astype(np.float32)
    return (np.array(o, dtype=np.int32), np.array([ks[0] for ks in cover], dtype=np.int32),
            np.array([len(ks) for ks in cover], dtype=np.int32), coef)


def plan(H, W, S, stride=None, win="hann"):
    stride = S // 2 if stride is None else stride
    w = window(win, S)
    oy, fy, cy, ky = axis(H, S, stride, w)
    ox, fx, cx, kx = axis(W, S, stride, w)
    return SimpleNamespace(H=H, W=W, S=S, stride=stride, window=win, w=w, oy=oy, ox=ox, ny=len(oy), nx=len(ox),
                           first_y=fy, count_y=cy, coef_y=ky, first_x=fx, count_x=cx, coef_x=kx)


def same_plan(p, q):
    """q (a tiling.TilePlan) holds exactly the tables of the restated plan p."""
    for k in ("oy", "ox", "first_y", "count_y", "coef_y", "first_x", "count_x", "coef_x"):
        a, b = getattr(p, k), getattr(q, k)
        if a.dtype != b.dtype or a.shape != b.shape or not np.array_equal(a, b):
            return False
    return (p.ny, p.nx) == (q.ny, q.nx)


def normalize_u8(u):
    """vg_gather_normalize_u8: (u/255 - 0.5)/0.5, each operation rounded to f32."""
    t = u.astype(np.float32) / f32(255.0)
    return ((t - f32(0.5)) / f32(0.5)).astype(np.float32)


def bf16_round(x):
    """f32 -> bf16 (round to nearest even) -> the uint16 bit patterns."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def gather(p, t0, B, CP, images_u8=None, images_f32=None):
    """-> f32 [B][S][S][CP] (pad channels zero): tiles [t0, t0 + B) from u8 [N][H][W][C] or f32 [N][C][H][W]."""
    S, per = p.S, p.ny * p.nx
    C = images_u8.shape[3] if images_u8 is not None else images_f32.shape[1]
    out = np.zeros((B, S, S, CP), dtype=np.float32)
    for b in range(B):
        t = t0 + b
        n, k = divmod(t, per)
        ky, kx = divmod(k, p.nx)
        y0, x0 = int(p.oy[ky]), int(p.ox[kx])
        if images_u8 is not None:
            out[b, :, :, :C] = normalize_u8(images_u8[n, y0:y0 + S, x0:x0 + S, :])
        else:
            out[b, :, :, :C] = np.transpose(images_f32[n, :, y0:y0 + S, x0:x0 + S], (1, 2, 0))
    return out


def blend_f32(p, tiles):
    """The contract, in f32 with every product and sum rounded on its own:
    out = ((0 + cy_0 inner_0) + cy_1 inner_1) + ...,  inner_ky = ((0 + cx_0 r_0) + cx_1 r_1) + ...  (ascending)."""
    S, per = p.S, p.ny * p.nx
    N, C = tiles.shape[0] // per, tiles.shape[1]
    r = tiles.astype(np.float32).reshape(N, p.ny, p.nx, C, S, S)
    out = np.zeros((N, C, p.H, p.W), dtype=np.float32)
    for y in range(p.H):
        for x in range(p.W):
            acc = np.zeros((N, C), dtype=np.float32)
            for jy in range(p.count_y[y]):
                ky = p.first_y[y] + jy
                inner = np.zeros((N, C), dtype=np.float32)
                for jx in range(p.count_x[x]):
                    kx = p.first_x[x] + jx
                    inner = (inner + (p.coef_x[x, jx] * r[:, ky, kx, :, y - p.oy[ky], x - p.ox[kx]]).astype(f32)).astype(f32)
                acc = (acc + (p.coef_y[y, jy] * inner).astype(f32)).astype(f32)
            out[:, :, y, x] = acc
    return out


def blend_f64(p, tiles):
    """sum_k wy wx r / sum_k wy wx in f64 from the window itself (no rounded coefficient enters)."""
    S, per = p.S, p.ny * p.nx
    N, C = tiles.shape[0] // per, tiles.shape[1]
    r = tiles.astype(np.float64).reshape(N, p.ny, p.nx, C, S, S)
    num = np.zeros((N, C, p.H, p.W))
    den = np.zeros((p.H, p.W))
    w2 = np.outer(p.w, p.w)
    for ky, y0 in enumerate(p.oy):
        for kx, x0 in enumerate(p.ox):
            num[:, :, y0:y0 + S, x0:x0 + S] += w2 * r[:, ky, kx]
            den[y0:y0 + S, x0:x0 + S] += w2
    return num / den


def with_tables(p, coef_y, coef_x):
    """p with hand-made coefficient tables (same origins and cover ranges; the tables may be wider than the cover)."""
    q = SimpleNamespace(**vars(p))
    q.coef_y, q.coef_x = np.ascontiguousarray(coef_y, dtype=np.float32), np.ascontiguousarray(coef_x, dtype=np.float32)
    return q


def dyadic_tables(p, width):
    """Coefficients m / 8 with sum 1 over each coordinate's cover (count <= 5 <= width): exact in f32 with small tiles."""
    rows = {1: [8], 2: [3, 5], 3: [1, 4, 3], 4: [1, 2, 4, 1], 5: [1, 2, 2, 2, 1]}

    def one(count):
        t = np.zeros((count.size, width), dtype=np.float32)
        for q, c in enumerate(count):
            t[q, :c] = np.array(rows[int(c)], dtype=np.float32) / f32(8)
        return t
    return with_tables(p, one(p.count_y), one(p.count_x))


def exact_tiles(T, C, S, seed=0):
    """Tile values in {+-1, +-2, +-3}."""
    rng = np.random.default_rng(seed)
    return (rng.integers(1, 4, size=(T, C, S, S)) * rng.choice([-1, 1], size=(T, C, S, S))).astype(np.float32)


def blend_bound(p, rmax):
    """|f32 blend - f64 blend| <= (cover_y + cover_x + 3) * 2^-24 * max|r|.  Counted from the roundings, u = 2^-24 the unit
    roundoff, a_j and b_i the exact normalised weights (positive, sum 1 per coordinate), m_x / m_y the cover counts:
      inner sum: term j carries the rounding of its coefficient (u), of its product (u) and of the additions it lives through,
      at most m_x - 1 (the first, 0 + t, is exact): relative (m_x + 1) u to first order, so
      |inner^ - inner| <= (m_x + 1) u sum_j a_j |r_j| <= (m_x + 1) u max|r|;
      outer sum: the same count with m_y, applied to inner values that are themselves below max|r|: (m_y + 1) u max|r|, plus the
      inner errors weighed by b_i (sum 1): first order in total (m_y + m_x + 2) u max|r|.
    Everything of second order is below ((m_y + m_x + 2) u)^2 max|r| < 2^-38 max|r| for covers <= 8, and the f64 restatement's
    own error is of order 2^-50: one further u covers both.  Hence k = 3."""
    return (int(p.count_y.max()) + int(p.count_x.max()) + 3) * 2.0 ** -24 * rmax
