"""numpy restatement of tiled denoising, written from include/vaegan_hip.h ("Tiled denoising") and the issue's contract, not
from tiling.py or csrc/tiling.hip: the plan (origins, cover ranges, normalised coefficients), the gather from both sources,
and the blend in the contract's order in f32, plus an f64 form that divides by the summed window instead of using the
rounded coefficients.  For the shapes past one workgroup: a slot-vectorised form of the f32 blend, the table of those cases
with what each is there for, and tables with one bad entry each together with the result the header's "Table safety" promises."""
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


def _blend_slots(p, tiles, table_safe):
    """blend_f32 with the loops turned inside out: a loop over the (jy, jx) table slots only, every slot one masked numpy
    pass over all (n, c, y, x).  Per pixel the slots are visited in the same ascending order and every product and every sum
    is rounded to f32 on its own, so the bits are those of the pixel loop.  table_safe applies the header's "Table safety"
    words, one per line below; without it the tables are asserted to need none of them."""
    S, per = p.S, p.ny * p.nx
    N, C = tiles.shape[0] // per, tiles.shape[1]
    wy, wx = p.coef_y.shape[1], p.coef_x.shape[1]
    r = tiles.astype(np.float32).reshape(N, p.ny, p.nx, C, S, S)
    first_y, first_x = p.first_y.astype(np.int64), p.first_x.astype(np.int64)
    oy, ox = p.oy.astype(np.int64), p.ox.astype(np.int64)
    cy = np.clip(p.count_y.astype(np.int64), 0, wy)                        # "count is clamped to [0, width]"
    cx = np.clip(p.count_x.astype(np.int64), 0, wx)
    if not table_safe:
        assert np.array_equal(cy, p.count_y) and np.array_equal(cx, p.count_x)
    yy, xx = np.arange(p.H, dtype=np.int64), np.arange(p.W, dtype=np.int64)

    def slot(first, count, o, n, q, j):
        """-> (use [L], tile index [L], local coordinate [L]) of slot j along one axis; unused entries index 0."""
        k = first + j
        use = j < count
        ok = (k >= 0) & (k < n)                                            # "a tile index outside [0, ny) / [0, nx) ..."
        loc = q - o[np.where(ok, k, 0)]
        ok &= (loc >= 0) & (loc < S)                                       # "... or a local coordinate outside [0, S) drops that term"
        assert table_safe or bool(np.all(ok[use]))
        use = use & ok
        return use, np.where(use, k, 0), np.where(use, loc, 0)

    acc = np.zeros((N, C, p.H, p.W), dtype=np.float32)
    for jy in range(wy):
        uy, ky, ly = slot(first_y, cy, oy, p.ny, yy, jy)
        if not uy.any():
            continue
        inner = np.zeros((N, C, p.H, p.W), dtype=np.float32)
        for jx in range(wx):
            ux, kx, lx = slot(first_x, cx, ox, p.nx, xx, jx)
            if not ux.any():
                continue
            v = r[:, ky[:, None], kx[None, :], :, ly[:, None], lx[None, :]]                 # [H, W, N, C]
            v = np.transpose(v, (2, 3, 0, 1))
            term = (p.coef_x[:, jx].astype(f32)[None, None, None, :] * v).astype(f32)
            inner = np.where(ux[None, None, None, :], (inner + term).astype(f32), inner)
        term = (p.coef_y[:, jy].astype(f32)[None, None, :, None] * inner).astype(f32)
        acc = np.where(uy[None, None, :, None], (acc + term).astype(f32), acc)
    return acc


def blend_f32_fast(p, tiles):
    """blend_f32, slot-vectorised (tests/test_tiling_cpu.py: the same bits), for the shapes the pixel loop is too slow for."""
    return _blend_slots(p, tiles, False)


def blend_f32_table_safe(p, tiles):
    """The f32 contract over tables that may hold bad entries, with the header's "Table safety" applied word for word: count
    clamped to [0, width]; a term whose tile index is outside [0, ny) / [0, nx), or whose local coordinate is outside [0, S),
    is dropped (the sum goes on with the next slot; a dropped ky drops its whole inner sum)."""
    return _blend_slots(p, tiles, True)


def gather_table_safe(p, t0, B, CP, images_u8=None, images_f32=None):
    """gather over origin tables that may hold bad entries: "an origin outside the image writes a zero tile"."""
    S, per = p.S, p.ny * p.nx
    bad_y, bad_x = (p.oy < 0) | (p.oy > p.H - S), (p.ox < 0) | (p.ox > p.W - S)
    q = SimpleNamespace(**vars(p))
    q.oy, q.ox = np.where(bad_y, 0, p.oy), np.where(bad_x, 0, p.ox)
    out = gather(q, t0, B, CP, images_u8=images_u8, images_f32=images_f32)
    for b in range(B):
        ky, kx = divmod((t0 + b) % per, p.nx)
        if bad_y[ky] or bad_x[kx]:
            out[b] = 0
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


# ---- the cases past one workgroup, and what each is there for ---------------------------------------------------------
# Launch geometry as include/vaegan_hip.h and the comments of csrc/tiling.hip state it: the gather runs workgroups of 64 x 4
# pixels of one tile, grid (B, ceil(S / 4), ceil(S / 64)); the blend gives a thread 4 consecutive x and a workgroup 64 such
# groups by 32 rows, grid (N C, ceil(H / 32), ceil(ceil(W / 4) / 64)); x tables wider than REG_WIDTH slots are read one float
# at a time (no group is "whole" then), and the store is one 16-byte vector only where W % 4 == 0.
GATHER_WG, BLEND_GROUP, BLEND_WG_X, BLEND_WG_Y, REG_WIDTH = (64, 4), 4, 64, 32, 4


def ceil_div(a, b):
    return -(-a // b)


def group_kinds(p):
    """-> (whole, straddling) counts of the blend's groups of 4 consecutive x, from the origins alone.  A group lies whole
    inside its tiles where its four x are in the image and are covered by the same tiles (each of those then holds all four);
    every other group straddles a tile edge or the image's."""
    def cover(x):
        return frozenset(k for k, o in enumerate(p.ox) if o <= x < o + p.S)
    whole = 0
    groups = ceil_div(p.W, BLEND_GROUP)
    for q in range(groups):
        xs = range(BLEND_GROUP * q, BLEND_GROUP * q + BLEND_GROUP)
        whole += xs[-1] < p.W and len({cover(x) for x in xs}) == 1
    return whole, groups - whole


def case_properties(p):
    """What a case of BLEND_CASES is there for, derived from the restated plan alone."""
    cover_y, cover_x = int(p.count_y.max()), int(p.count_x.max())
    return dict(tiles=(p.ny, p.nx), cover=(cover_y, cover_x),
                groups=group_kinds(p) if cover_x <= REG_WIDTH else None,           # None: every group reads scalars
                blend_grid=(ceil_div(p.H, BLEND_WG_Y), ceil_div(ceil_div(p.W, BLEND_GROUP), BLEND_WG_X)),
                gather_grid=(ceil_div(p.S, GATHER_WG[1]), ceil_div(p.S, GATHER_WG[0])),
                vector_store=p.W % 4 == 0)


# (H, W, S, stride) -> the properties above, written down by hand; tests/test_tiling_cpu.py holds them against
# case_properties(plan(...)), so that the table cannot drift to shapes that no longer reach the path.  Each is the smallest
# shape that reaches its path.
BLEND_CASES = {
    (9, 260, 8, 4): dict(tiles=(2, 64), cover=(2, 2), groups=(65, 0), blend_grid=(1, 2), gather_grid=(2, 1), vector_store=True),
    (9, 261, 8, 3): dict(tiles=(2, 86), cover=(2, 4), groups=(0, 66), blend_grid=(1, 2), gather_grid=(2, 1), vector_store=False),
    (9, 517, 8, 4): dict(tiles=(2, 129), cover=(2, 3), groups=(128, 2), blend_grid=(1, 3), gather_grid=(2, 1), vector_store=False),
    (40, 300, 8, 5): dict(tiles=(8, 60), cover=(3, 3), groups=(1, 74), blend_grid=(2, 2), gather_grid=(2, 1), vector_store=True),
    # the widest register table, in the second workgroup too
    (11, 264, 8, 2): dict(tiles=(3, 129), cover=(3, 4), groups=(0, 66), blend_grid=(1, 2), gather_grid=(2, 1), vector_store=True),
    # x tables of 5 to 8 slots: scalar reads, with the 16-byte store ...
    (12, 24, 8, 1): dict(tiles=(5, 17), cover=(5, 8), groups=None, blend_grid=(1, 1), gather_grid=(2, 1), vector_store=True),
    # ... with scalar stores and VG_TILE_MAX_COVER on both axes ...
    (16, 15, 8, 1): dict(tiles=(9, 8), cover=(8, 8), groups=None, blend_grid=(1, 1), gather_grid=(2, 1), vector_store=False),
    # ... and at another tile size
    (32, 36, 16, 2): dict(tiles=(9, 11), cover=(8, 8), groups=None, blend_grid=(1, 1), gather_grid=(4, 1), vector_store=True),
    # the engines' tile sizes: a flush tile at an odd origin, so whole and straddling groups share a launch
    (101, 83, 64, 32): dict(tiles=(3, 2), cover=(3, 2), groups=(19, 2), blend_grid=(4, 1), gather_grid=(16, 1), vector_store=False),
    (150, 203, 128, 64): dict(tiles=(2, 3), cover=(2, 3), groups=(49, 2), blend_grid=(5, 1), gather_grid=(32, 2), vector_store=False),
    (259, 261, 256, 128): dict(tiles=(2, 2), cover=(2, 2), groups=(64, 2), blend_grid=(9, 2), gather_grid=(64, 4), vector_store=False),
}

# (H, W, S): two images each a few pixels larger than the engine's tile, default stride: odd flush origins on both axes
GATHER_CASES = {(101, 83, 64): dict(oy=[0, 32, 37], ox=[0, 19], gather_grid=(16, 1)),
                (131, 133, 128): dict(oy=[0, 3], ox=[0, 5], gather_grid=(32, 2)),
                (259, 261, 256): dict(oy=[0, 3], ox=[0, 5], gather_grid=(64, 4))}


def uniform_tiles(p, N, C, seed):
    """Tiles uniform in [-1, 1] from a seeded generator, f32 [N ny nx, C, S, S]."""
    return np.random.default_rng(seed).uniform(-1, 1, size=(N * p.ny * p.nx, C, p.S, p.S)).astype(np.float32)


# ---- tables with bad entries ---------------------------------------------------------------------------------------
def safety_plan(path):
    """"reg": x table of at most REG_WIDTH slots, every group of 4 x whole (origins and S multiples of 4); "wide": 8 slots."""
    return plan(13, 36, 8, 4) if path == "reg" else plan(12, 24, 8, 1)


def _edited(p, **tables):
    q = SimpleNamespace(**vars(p))
    for k in ("oy", "ox", "first_y", "count_y", "coef_y", "first_x", "count_x", "coef_x"):
        setattr(q, k, np.array(tables.get(k, getattr(p, k))))
    return q


def _arm(coef, rows):
    """Every slot of the rows gets a non-zero dyadic coefficient, so that a term that should have been dropped shows."""
    coef[rows, :] = (0.5 ** np.arange(1, coef.shape[1] + 1)).astype(np.float32)


def blend_table_edits(p, C):
    """-> {name: (edited plan, reach)}: p with ONE kind of bad entry each, every entry off by one.  reach = how many floats
    before or behind the tile buffer the furthest address lies that a kernel WITHOUT the check for that entry could form from
    it (the tests keep at least that many guard floats there); derivations per entry below, SS = S * S, the tile of (n, ky,
    kx, c) starting at ((n ny nx + ky nx + kx) C + c) SS.  An origin table read at index -1 or at its length (1 element past
    either end) is the only table access a missing check can displace, bar the coefficient noted at count = width + 1.
    p.W % 4 == 0: the x edits take whole groups of four."""
    S, SS, H, W = p.S, p.S * p.S, p.H, p.W
    wy, wx = p.coef_y.shape[1], p.coef_x.shape[1]
    lo_x, hi_x, lo_y, hi_y = slice(0, 4), slice(W - 4, W), slice(0, 2), slice(H - 2, H)
    assert W % 4 == 0 and wy >= 2 and wx >= 2 and np.all(p.first_x[lo_x] == 0) and np.all(p.first_y[lo_y] == 0)
    assert np.all((p.first_x + p.count_x)[hi_x] == p.nx) and np.all((p.first_y + p.count_y)[hi_y] == p.ny)
    out = {}

    def axis_edit(first, count, coef, rows, width, below):
        first, count, coef = first.copy(), count.copy(), coef.copy()
        if below:
            first[rows] = -1                                              # slot 0 -> tile -1; the later slots stay real tiles
        count[rows] = np.minimum(count[rows] + 1, width)                  # above: the last slot -> tile n, one past the end
        _arm(coef, rows)
        return first, count, coef

    # kx = -1: tile (ky, -1) is one tile before (ky, 0): at most C SS floats before the buffer (n = ky = c = 0)
    f, c, k = axis_edit(p.first_x, p.count_x, p.coef_x, lo_x, wx, True)
    out["first_x=-1"] = (_edited(p, first_x=f, count_x=c, coef_x=k), C * SS)
    # kx = nx: tile (ky, nx) is tile (ky + 1, 0): at most C SS floats behind the buffer (the last n and ky)
    f, c, k = axis_edit(p.first_x, p.count_x, p.coef_x, hi_x, wx, False)
    assert np.all((f + c)[hi_x] == p.nx + 1)
    out["first_x+count=nx+1"] = (_edited(p, first_x=f, count_x=c, coef_x=k), C * SS)
    # ky = -1: a whole tile row before (0, kx): at most nx C SS floats before the buffer
    f, c, k = axis_edit(p.first_y, p.count_y, p.coef_y, lo_y, wy, True)
    out["first_y=-1"] = (_edited(p, first_y=f, count_y=c, coef_y=k), p.nx * C * SS)
    # ky = ny: the tile row behind the last: at most nx C SS floats behind the buffer
    f, c, k = axis_edit(p.first_y, p.count_y, p.coef_y, hi_y, wy, False)
    assert np.all((f + c)[hi_y] == p.ny + 1)
    out["first_y+count=ny+1"] = (_edited(p, first_y=f, count_y=c, coef_y=k), p.nx * C * SS)
    # count = width + 1: the tables one slot narrower than the cover.  Unclamped, slot `width` is a real covering tile (nothing
    # leaves the tile buffer) weighed with coef[p][width], the next row's slot 0, or 1 float behind the table for the last row
    assert int(p.count_x.max()) == wx and int(p.count_y.max()) == wy
    out["count_x=width+1"] = (_edited(p, coef_x=p.coef_x[:, :wx - 1]), 0)
    out["count_y=width+1"] = (_edited(p, coef_y=p.coef_y[:, :wy - 1]), 0)
    # count < 0: clamped to 0, the element is 0.  Nothing is read at all.
    cx, cy = p.count_x.copy(), p.count_y.copy()
    cx[4:8], cy[2] = -1, -1
    out["count=-1"] = (_edited(p, count_x=cx, count_y=cy), 0)
    # lx = -1 at x = 0 (origin 0 moved to 1): 1 float before the tile row, so before the buffer for the first row of tile 0
    ox = p.ox.copy()
    ox[0] = 1
    out["lx=-1"] = (_edited(p, ox=ox), 1)
    # lx = S at x = W - 1 (the flush origin moved down by 1): 1 float behind the last row of the last tile
    ox = p.ox.copy()
    ox[-1] = W - S - 1
    out["lx=S"] = (_edited(p, ox=ox), 1)
    # ly = -1 at y = 0: one tile row (S floats) before the tile;  ly = S at y = H - 1: the row behind the tile's last, S floats
    oy = p.oy.copy()
    oy[0] = 1
    out["ly=-1"] = (_edited(p, oy=oy), S)
    oy = p.oy.copy()
    oy[-1] = H - S - 1
    out["ly=S"] = (_edited(p, oy=oy), S)
    return out


BLEND_EDIT_NAMES = ("first_x=-1", "first_x+count=nx+1", "first_y=-1", "first_y+count=ny+1", "count_x=width+1", "count_y=width+1",
                    "count=-1", "lx=-1", "lx=S", "ly=-1", "ly=S")


def gather_origin_edits(p):
    """-> {name: (edited plan, reach)}: one origin just off the image each.  reach in PIXELS of one channel plane (f32 source;
    times C bytes for the u8 source) before or behind the image set that a kernel without the check would read: a row for y
    (the first row of image 0 / the row behind the last of the last image), one pixel for x."""
    out = {}
    for name, key, idx, val, reach in (("oy=-1", "oy", 0, -1, p.W), ("oy=H-S+1", "oy", -1, p.H - p.S + 1, p.W),
                                       ("ox=-1", "ox", 0, -1, 1), ("ox=W-S+1", "ox", -1, p.W - p.S + 1, 1)):
        o = getattr(p, key).copy()
        o[idx] = val
        out[name] = (_edited(p, **{key: o}), reach)
    return out


GATHER_EDIT_NAMES = ("oy=-1", "oy=H-S+1", "ox=-1", "ox=W-S+1")


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
