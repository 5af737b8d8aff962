"""GPU: tiled denoising (vg_tile_gather, vg_tile_blend, and denoise_tiled / tiled_denoise_eval / tiled_test_epoch above them)
against the numpy restatement tests/_tiling_ref.py.  The gather and the exact-input blends (tests/test_tiling_cpu.py shows
that every product and partial sum of theirs is an f32 number) are compared bit for bit; random inputs within the bound
counted from the roundings (_tiling_ref.blend_bound).  No expectation is taken from the kernel under test.  Every kernel
output is a NaN-filled slice of a larger NaN-filled buffer: a stale right answer in recycled memory cannot pass, and a store
before or past the output shows in the guard rows.
Beyond the small shapes: the blend past one workgroup along x and y and over every table width (the cases of
_tiling_ref.BLEND_CASES, whose reasons tests/test_tiling_cpu.py asserts), the gather at the engines' tile sizes 64, 128, 256
and with pixels of two 16-byte units, the header's "Table safety" promise entry by entry, a graph replay, and S = 128 end to
end.  Not covered: S = 256 end to end, table entries of large magnitude, and tensors of more than 2^31 elements (the 64-bit
offsets of the blend): the first two for the reasons given at their tests, the last because it needs gigabytes per case."""
import numpy as np
import pytest
import torch

import _tiling_ref as R
import vaegan_amd as V

pytestmark = pytest.mark.gpu
DEV = "cuda"
ops, G, T = V.ops, V.geometry, V.tiling
PAD = 64                                               # guard elements on either side (a multiple of 16 bytes in f32 and bf16)


def guarded(numel, dtype=torch.float32, shift=0):
    """(buffer, its NaN-filled middle of numel elements); shift moves the middle off 16-byte alignment."""
    buf = torch.full((numel + 2 * PAD + shift,), float("nan"), dtype=dtype, device=DEV)
    return buf, buf[PAD + shift:PAD + shift + numel]


def guards_intact(buf, numel, shift=0):
    return bool(torch.isnan(buf[:PAD + shift]).all() and torch.isnan(buf[PAD + shift + numel:]).all())


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def act_bits(t, dt):
    """An engine tensor's bit patterns on the host (bf16 as uint16)."""
    return t.view(torch.int16).cpu().numpy().view(np.uint16) if dt == G.BF16 else bits(t.cpu().numpy())


def want_bits(x, dt):
    return R.bf16_round(x) if dt == G.BF16 else bits(x.astype(np.float32))


def device_plan(p):
    """A tiling.TilePlan that holds exactly the restated (or hand-made) tables of p."""
    return T.TilePlan(p.H, p.W, p.S, p.stride, p.window, p.oy, p.ox, p.first_y, p.count_y, p.coef_y, p.first_x, p.count_x, p.coef_x)


def blend(p, tiles, N, C, shift=0):
    """ops.tile_blend over a guarded NaN-filled output -> host f32 [N,C,H,W]."""
    n = N * C * p.H * p.W
    buf, out = guarded(n, shift=shift)
    got = ops.tile_blend(torch.from_numpy(tiles).to(DEV), device_plan(p), out=out.view(N, C, p.H, p.W))
    assert got.data_ptr() == out.data_ptr() and guards_intact(buf, n, shift)
    return got.cpu().numpy()


# ---- gather -------------------------------------------------------------------------------------------------------
GH, GW, GS, GSTRIDE = 13, 11, 8, 3                      # y origins 0, 3, 5; x origins 0, 3 (odd): 6 tiles per image


@pytest.mark.parametrize("dt", [G.F32, G.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("src", ["u8", "f32"])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("t0,B", [(0, 12), (4, 5)], ids=["all", "straddle_short"])
def test_gather_equals_the_restatement_and_the_existing_kernels(dt, src, C, t0, B):
    """N = 2: tiles [4, 9) straddle the two images (image 0 ends at tile 5) and end short of the list."""
    p = R.plan(GH, GW, GS, GSTRIDE)
    assert p.ox.tolist() == [0, 3] and p.oy.tolist() == [0, 3, 5]
    plan = T.tile_plan(GH, GW, GS, GSTRIDE)
    rng = np.random.default_rng(100 * C + t0)
    CP = G.padc(C, dt)
    if src == "u8":
        host = rng.integers(0, 256, size=(2, GH, GW, C), dtype=np.uint8)
        host[0, 0, 0, :], host[1, -1, -1, :] = 0, 255
        want = R.gather(p, t0, B, CP, images_u8=host)
    else:
        host = rng.uniform(-1, 1, size=(2, C, GH, GW)).astype(np.float32)
        want = R.gather(p, t0, B, CP, images_f32=host)
    images = torch.from_numpy(host).to(DEV)
    n = B * GS * GS * CP
    buf, out = guarded(n, ops.TORCH_DT[dt])
    got = ops.tile_gather(images, plan, t0, B, CP, dt, out=out.view(B, GS, GS, CP))
    assert guards_intact(buf, n)
    gb = act_bits(got, dt)
    assert np.array_equal(gb, want_bits(want, dt))
    assert not np.any(gb[..., C:])                                        # pad channels are zero bits
    # ... and equals vg_gather_normalize_u8 + vg_nchw_to_nhwc of the cropped tile
    for b in range(B):
        n_img, k = divmod(t0 + b, p.ny * p.nx)
        ky, kx = divmod(k, p.nx)
        y0, x0 = int(p.oy[ky]), int(p.ox[kx])
        if src == "u8":
            crop = images[n_img, y0:y0 + GS, x0:x0 + GS, :].contiguous()[None]
            x = ops.gather_normalize_u8(crop, torch.zeros(1, dtype=torch.int64, device=DEV))
        else:
            x = images[n_img:n_img + 1, :, y0:y0 + GS, x0:x0 + GS].contiguous()
        ref = ops.nchw_to_nhwc(x, CP, dt)
        assert np.array_equal(act_bits(ref, dt)[0], gb[b]), b


# ---- blend, exact inputs, bit for bit -------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,stride,window,shift", [
    (8, 8, 4, "hann", 0),                               # one tile: the output is the tile
    (20, 12, 4, "tri", 0),                              # dyadic tables, W % 4 == 0: 16-byte stores
    (20, 12, 4, "tri", 1),                              # the same through the scalar stores (out off 16-byte alignment)
    (19, 13, 8, "box", 0)])                             # the flush tile, coefficients 1/2; W % 4 == 1
def test_blend_exact_inputs_bitwise(H, W, stride, window, shift):
    p = R.plan(H, W, 8, stride, window)
    N, C = 2, 3
    tiles = R.exact_tiles(N * p.ny * p.nx, C, 8, seed=H + W)
    got = blend(p, tiles, N, C, shift)
    assert np.array_equal(bits(got), bits(R.blend_f32(p, tiles)))
    if (H, W) == (8, 8):
        assert np.array_equal(bits(got), bits(tiles.reshape(N, C, 8, 8)))
    again = blend(p, tiles, N, C, shift)                                   # two launches: identical bits
    assert np.array_equal(bits(again), bits(got))


def test_blend_hand_made_dyadic_tables_cover_5():
    """(23, 9), stride 2: up to 5 tiles cover a row; tables of width 5 on both axes (the x axis uses 2 slots, the rest 0)."""
    p = R.dyadic_tables(R.plan(23, 9, 8, 2, "tri"), 5)
    assert int(p.count_y.max()) == 5 and p.coef_x.shape[1] == 5 and 9 % 4 != 0
    N, C = 2, 1
    tiles = R.exact_tiles(N * p.ny * p.nx, C, 8, seed=7)
    got = blend(p, tiles, N, C)
    assert np.array_equal(bits(got), bits(R.blend_f32(p, tiles)))
    assert np.array_equal(bits(blend(p, tiles, N, C)), bits(got))


# ---- blend, random inputs -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(13, 37), (37, 13), (12, 24)])
def test_blend_random_inputs_within_the_counted_bound(H, W):
    """hann, stride 3, tiles uniform in [-1, 1] against the f64 restatement.  (13, 37): tables 3 wide, W % 4 == 1; (37, 13):
    more rows than one workgroup takes; (12, 24): x table 4 wide with 16-byte stores.  The odd origins make most groups of
    four x straddle a tile edge, some lie whole inside their tiles: both read paths run.
    Bound: (cover_y + cover_x + k) 2^-24 max|r| with k = 3 (derivation: _tiling_ref.blend_bound): (3 + 3 + 3) 2^-24 = 5.36e-7,
    (3 + 4 + 3) 2^-24 = 5.96e-7 for |r| <= 1.  Measured on the MI355X: 8.5e-8, 1.04e-7, 1.05e-7."""
    p = R.plan(H, W, 8, 3, "hann")
    N, C = 2, 3
    tiles = np.random.default_rng(11).uniform(-1, 1, size=(N * p.ny * p.nx, C, 8, 8)).astype(np.float32)
    got = blend(p, tiles, N, C)
    err = np.abs(got.astype(np.float64) - R.blend_f64(p, tiles)).max()
    bound = R.blend_bound(p, float(np.abs(tiles).max()))
    print("blend vs f64:", (H, W), "max error", err, "bound", bound)
    assert err <= bound
    # the contract fixes the order and rounds every product and sum on its own: the f32 restatement is met bit for bit (the
    # exact-input cases cannot see a product fused into a sum; this one can)
    assert np.array_equal(bits(got), bits(R.blend_f32(p, tiles)))


def test_round_trip_gather_then_blend_returns_the_image():
    """f32 image -> vg_tile_gather -> vg_nhwc_to_nchw (no tanh) -> vg_tile_blend: every covering tile holds the pixel itself,
    so the blend returns it within the counted bound (the coefficients of a pixel sum to 1 only within their roundings).
    (37, 29), stride 3, hann.  Measured on the MI355X: 1.19e-7 = 1 ulp of 1.0; bound (3 + 4 + 3) 2^-24 max|img| = 5.36e-7."""
    H, W, S = 37, 29, 8
    p, plan = R.plan(H, W, S, 3, "hann"), T.tile_plan(H, W, S, 3, "hann")
    N, C = 2, 3
    img = np.random.default_rng(3).uniform(-1, 1, size=(N, C, H, W)).astype(np.float32)
    Tn = N * p.ny * p.nx
    tiles = torch.full((Tn, C, S, S), float("nan"), dtype=torch.float32, device=DEV)
    x = torch.from_numpy(img).to(DEV)
    for t0 in range(0, Tn, 50):                                            # chunks of 50 tiles, the last one short
        b = min(50, Tn - t0)
        ops.nhwc_to_nchw(ops.tile_gather(x, plan, t0, b, 4, G.F32), C, G.F32, out=tiles[t0:t0 + b])
    assert np.array_equal(tiles.cpu().numpy().reshape(N, p.ny, p.nx, C, S, S)[1, 2, 1], img[1, :, 6:14, 3:11])
    buf, out = guarded(img.size)
    got = ops.tile_blend(tiles, plan, out=out.view(N, C, H, W)).cpu().numpy()
    assert guards_intact(buf, img.size)
    err = np.abs(got.astype(np.float64) - img).max()
    print("round trip: max error", err, "bound", R.blend_bound(p, float(np.abs(img).max())))
    assert err <= R.blend_bound(p, float(np.abs(img).max()))


# ---- blend past one workgroup and over the whole table width ---------------------------------------------------------
def case_id(c):
    return "x".join(map(str, c))


WIDE_CASES = [(c, 0) for c in R.BLEND_CASES] + [(c, 1) for c, q in R.BLEND_CASES.items() if q["vector_store"]]


@pytest.mark.parametrize("case,shift", WIDE_CASES, ids=[case_id(c) + ("_shifted" if s else "") for c, s in WIDE_CASES])
def test_blend_past_one_workgroup_and_over_the_whole_table_width(case, shift):
    """Every case of _tiling_ref.BLEND_CASES (tests/test_tiling_cpu.py asserts what each reaches: a second and third workgroup
    along x, a second to ninth along y, x tables of 2 to 8 slots, whole and straddling groups in one launch at S = 64, 128,
    256), hann, N = 2 (1 at S = 256), C = 3, tiles uniform in [-1, 1]: bit for bit against the f32 restatement, within the
    counted bound of the f64 one, guards intact, a second launch the same bits.  The W % 4 == 0 cases run again with the
    output off 16-byte alignment: the scalar stores on the data of the vector stores.
    Bound (cover_y + cover_x + 3) 2^-24 max|r| (_tiling_ref.blend_bound).  Measured on the MI355X, error / bound in the
    table's order: 0.30, 0.23, 0.30, 0.21, 0.21, 0.14, 0.097, 0.10, 0.26, 0.27, 0.29 (errors 1.1e-7 to 1.4e-7; the shifted
    runs give the figures of the unshifted ones, being the same bits)."""
    H, W, S, stride = case
    p = R.plan(H, W, S, stride)
    N, C = (1 if S == 256 else 2), 3
    tiles = R.uniform_tiles(p, N, C, seed=H + W)
    got = blend(p, tiles, N, C, shift)
    err = np.abs(got.astype(np.float64) - R.blend_f64(p, tiles)).max()
    bound = R.blend_bound(p, float(np.abs(tiles).max()))
    print("blend vs f64:", case, "shift", shift, "max error", err, "bound", bound, "ratio", err / bound)
    assert np.array_equal(bits(got), bits(R.blend_f32_fast(p, tiles)))
    assert err <= bound
    assert np.array_equal(bits(blend(p, tiles, N, C, shift)), bits(got))


# ---- gather at every engine's tile size ------------------------------------------------------------------------------
def gather_source(src, N, C, H, W, seed):
    rng = np.random.default_rng(seed)
    if src == "u8":
        host = rng.integers(0, 256, size=(N, H, W, C), dtype=np.uint8)
        host[0, 0, 0, :], host[-1, -1, -1, :] = 0, 255
        return host, dict(images_u8=host)
    host = rng.uniform(-1, 1, size=(N, C, H, W)).astype(np.float32)
    return host, dict(images_f32=host)


@pytest.mark.parametrize("dt", [G.F32, G.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("src", ["u8", "f32"])
@pytest.mark.parametrize("case", list(R.GATHER_CASES), ids=case_id)
def test_gather_at_the_engines_tile_sizes(case, src, dt):
    """S = 64, 128, 256 (grid.z 1, 2, 4), two images a few pixels larger than S with odd flush origins on both axes; the chunk
    is the last two tiles of image 0 and the first of image 1: it straddles the images and ends short of the list."""
    H, W, S = case
    p, plan = R.plan(H, W, S), T.tile_plan(H, W, S)
    per, C = p.ny * p.nx, 3
    t0, B, CP = per - 2, 3, G.padc(C, dt)
    host, kw = gather_source(src, 2, C, H, W, seed=S)
    want = R.gather(p, t0, B, CP, **kw)
    images = torch.from_numpy(host).to(DEV)
    n = B * S * S * CP
    buf, out = guarded(n, ops.TORCH_DT[dt])
    got = ops.tile_gather(images, plan, t0, B, CP, dt, out=out.view(B, S, S, CP))
    assert guards_intact(buf, n)
    gb = act_bits(got, dt)
    assert np.array_equal(gb, want_bits(want, dt))
    assert not np.any(gb[..., C:])                                        # pad channels are zero bits
    for b in (0, 1, 2):                                                    # first, last of image 0, first of image 1 (= last)
        n_img, k = divmod(t0 + b, per)
        assert n_img == (b == 2)
        ky, kx = divmod(k, p.nx)
        y0, x0 = int(p.oy[ky]), int(p.ox[kx])
        if src == "u8":
            crop = images[n_img, y0:y0 + S, x0:x0 + S, :].contiguous()[None]
            x = ops.gather_normalize_u8(crop, torch.zeros(1, dtype=torch.int64, device=DEV))
        else:
            x = images[n_img:n_img + 1, :, y0:y0 + S, x0:x0 + S].contiguous()
        assert np.array_equal(act_bits(ops.nchw_to_nhwc(x, CP, dt), dt)[0], gb[b]), b


@pytest.mark.parametrize("src", ["u8", "f32"])
@pytest.mark.parametrize("dt,C,CP", [(G.F32, 5, 8), (G.BF16, 9, 16)], ids=["f32_C5_CP8", "bf16_C9_CP16"])
def test_gather_of_pixels_wider_than_one_16_byte_unit(dt, C, CP, src):
    """Two trips of the channel loop; the pad channels are in the last unit only, next to a real channel."""
    p, plan = R.plan(GH, GW, GS, GSTRIDE), T.tile_plan(GH, GW, GS, GSTRIDE)
    assert G.per16(dt) < C < CP == 2 * G.per16(dt)
    t0, B = 4, 5
    host, kw = gather_source(src, 2, C, GH, GW, seed=C)
    want = R.gather(p, t0, B, CP, **kw)
    n = B * GS * GS * CP
    buf, out = guarded(n, ops.TORCH_DT[dt])
    got = ops.tile_gather(torch.from_numpy(host).to(DEV), plan, t0, B, CP, dt, out=out.view(B, GS, GS, CP))
    assert guards_intact(buf, n)
    gb = act_bits(got, dt)
    assert np.array_equal(gb[..., :C], want_bits(want, dt)[..., :C]) and np.any(gb[..., C - 1])
    assert not np.any(gb[..., C:])                                        # every pad channel is zero bits


# ---- table safety ---------------------------------------------------------------------------------------------------
L = ops.L                                                # the ctypes face of the library: the C entry points themselves
TABLE_PAD = 16                                           # guard elements around every table (the furthest table access is 1 out)


def guarded_table(a, before, after):
    """A host table inside a sentinel-filled device allocation -> (allocation, its host image, the table's slice)."""
    a = np.ascontiguousarray(a)
    host = np.concatenate([np.full(TABLE_PAD, before, a.dtype), a.ravel(), np.full(TABLE_PAD, after, a.dtype)])
    buf = torch.from_numpy(host).to(DEV)
    return buf, host, buf[TABLE_PAD:TABLE_PAD + a.size]


def guarded_tables(q):
    """The eight tables of q in guarded device memory.  Sentinels: an origin read one before its table is 0 and one behind it
    is the flush origin L - S, so that the local coordinate formed from it is a valid one and cannot hide a missing tile-index
    check behind the local-coordinate check; coefficients NaN; first / count (indexed by the coordinate only) 0."""
    nan = float("nan")
    spec = dict(oy=(0, q.H - q.S), ox=(0, q.W - q.S), first_y=(0, 0), count_y=(0, 0), first_x=(0, 0), count_x=(0, 0),
                coef_y=(nan, nan), coef_x=(nan, nan))
    return {k: guarded_table(getattr(q, k), *spec[k]) for k in spec}


def tables_untouched(tabs):
    return all(np.array_equal(bits(buf.cpu().numpy()), bits(host)) for buf, host, _ in tabs.values())


@pytest.mark.parametrize("edit", R.BLEND_EDIT_NAMES)
@pytest.mark.parametrize("path", ["reg", "wide"])
def test_blend_gives_the_promised_result_for_bad_table_entries(path, edit):
    """include/vaegan_hip.h, "Table safety": count clamped to [0, width]; a tile index outside [0, ny) / [0, nx) or a local
    coordinate outside [0, S) drops the term.  One kind of bad entry per case (_tiling_ref.blend_table_edits), over the x
    tables held in registers ("reg": every group whole, so the check of the whole-group path has to refuse and the scalar
    path has to drop) and the wide ones read one float at a time.  Expected: the restatement applying those words.
    Every bad entry is off by one, and the tile buffer, the output and the tables are slices of larger allocations whose
    guards reach at least as far as the furthest address a kernel without that check could form from the entry (reach, worked
    out per entry in blend_table_edits, computed by an unchecked host emulation in tests/test_tiling_cpu.py, and held against
    the guard below).  Such a kernel reads a NaN guard or a neighbouring tile and fails the comparison; it does not leave its
    allocations.  Left out: entries whose unchecked address has no such bound -- large magnitudes like INT_MAX, where
    first + j or the offset arithmetic itself may wrap."""
    p = R.safety_plan(path)
    N, C, S = 2, 2, p.S
    q, reach = R.blend_table_edits(p, C)[edit]
    tiles = R.uniform_tiles(p, N, C, seed=41)
    want = R.blend_f32_table_safe(q, tiles)
    guard = (p.nx + 1) * C * S * S                                         # floats on either side of the tile buffer
    assert reach <= guard
    tbuf = torch.full((tiles.size + 2 * guard,), float("nan"), dtype=torch.float32, device=DEV)
    tdev = tbuf[guard:guard + tiles.size]
    tdev.copy_(torch.from_numpy(tiles).reshape(-1))
    tabs = guarded_tables(q)
    ptr = {k: v[2].data_ptr() for k, v in tabs.items()}
    n = N * C * p.H * p.W
    obuf, out = guarded(n)
    L.check(L.load().vg_tile_blend(tdev.data_ptr(), out.data_ptr(), N, C, p.H, p.W, S, p.ny, p.nx, ptr["oy"], ptr["ox"],
                                   ptr["first_y"], ptr["count_y"], ptr["coef_y"], q.coef_y.shape[1], ptr["first_x"],
                                   ptr["count_x"], ptr["coef_x"], q.coef_x.shape[1], L.stream_ptr()), "vg_tile_blend")
    got = out.cpu().numpy().reshape(N, C, p.H, p.W)
    assert guards_intact(obuf, n) and tables_untouched(tabs)
    assert bool(torch.isnan(tbuf[:guard]).all() and torch.isnan(tbuf[guard + tiles.size:]).all())
    assert np.isfinite(got).all(), np.argwhere(~np.isfinite(got))[:4]
    assert np.array_equal(bits(got), bits(want)), np.argwhere(bits(got) != bits(want))[:4]


@pytest.mark.parametrize("edit", R.GATHER_EDIT_NAMES)
@pytest.mark.parametrize("src", ["u8", "f32"])
def test_gather_writes_a_zero_tile_for_an_origin_off_the_image(src, edit):
    """"An origin outside the image writes a zero tile": one origin at -1 or L - S + 1 per case (both axes), all 12 tiles of two
    images gathered; the tiles of that origin are zero bits, the others what they were.  The image set is a slice of a larger
    allocation (NaN for f32, 255 for u8) with 2 W C elements on either side: a kernel without the check reads at most one row
    (W pixels; C bytes each in the u8 set) before image 0 or behind the last image, and writes a non-zero tile."""
    p = R.plan(GH, GW, GS, GSTRIDE)
    q, reach = R.gather_origin_edits(p)[edit]
    N, C, CP, B = 2, 3, 4, 12
    host, kw = gather_source(src, N, C, GH, GW, seed=5)
    want = R.gather_table_safe(q, 0, B, CP, **kw)
    guard = 2 * GW * C
    assert reach * (C if src == "u8" else 1) <= guard
    sbuf = torch.full((host.size + 2 * guard,), 255 if src == "u8" else float("nan"),
                      dtype=torch.uint8 if src == "u8" else torch.float32, device=DEV)
    sdev = sbuf[guard:guard + host.size]
    sdev.copy_(torch.from_numpy(host).reshape(-1))
    oy, ox = guarded_table(q.oy, 0, GH - GS), guarded_table(q.ox, 0, GW - GS)
    n = B * GS * GS * CP
    obuf, out = guarded(n)
    L.check(L.load().vg_tile_gather(sdev.data_ptr() if src == "u8" else None, None if src == "u8" else sdev.data_ptr(), N, C, GH, GW,
                                    GS, p.ny, p.nx, oy[2].data_ptr(), ox[2].data_ptr(), 0, B, out.data_ptr(), CP, G.F32,
                                    L.stream_ptr()), "vg_tile_gather")
    got = out.cpu().numpy().reshape(B, GS, GS, CP)
    assert guards_intact(obuf, n) and tables_untouched(dict(oy=oy, ox=ox))
    assert np.array_equal(bits(got), bits(want))
    zero = [b for b in range(B) if not bits(got[b]).any()]
    assert len(zero) == {"oy": 2 * p.nx, "ox": 2 * p.ny}[edit[:2]]


# ---- graph replay ---------------------------------------------------------------------------------------------------
def test_gather_and_blend_replay_from_a_graph():
    """(101, 83), S = 64, stride 32, N = 2: vg_tile_gather -> vg_nhwc_to_nchw -> vg_tile_blend captured on one side stream into
    NaN-filled buffers (the tables uploaded by the eager run before).  One replay gives the eager bits, which are those of the
    restatement: the gather copies, the blend of the copied tiles in f32."""
    H, W, S, stride = 101, 83, 64, 32
    p, plan = R.plan(H, W, S, stride), T.tile_plan(H, W, S, stride)
    N, C, CP = 2, 3, 4
    Tn = N * p.ny * p.nx
    img = np.random.default_rng(9).uniform(-1, 1, size=(N, C, H, W)).astype(np.float32)
    x = torch.from_numpy(img).to(DEV)
    nan = float("nan")

    def run(nhwc, tiles, out):
        ops.tile_gather(x, plan, 0, Tn, CP, G.F32, out=nhwc)
        ops.nhwc_to_nchw(nhwc, C, G.F32, out=tiles)
        return ops.tile_blend(tiles, plan, out=out)

    def buffers():
        return (torch.full((Tn, S, S, CP), nan, device=DEV), torch.full((Tn, C, S, S), nan, device=DEV), guarded(img.size))
    nhwc, tiles, (buf, out) = buffers()
    eager = run(nhwc, tiles, out.view(N, C, H, W)).cpu().numpy()
    assert guards_intact(buf, img.size)
    want_tiles = np.ascontiguousarray(np.transpose(R.gather(p, 0, Tn, CP, images_f32=img)[..., :C], (0, 3, 1, 2)))
    assert np.array_equal(bits(tiles.cpu().numpy()), bits(want_tiles))
    assert np.array_equal(bits(eager), bits(R.blend_f32_fast(p, want_tiles)))
    nhwc_g, tiles_g, (buf_g, out_g) = buffers()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):                                       # one stream, no parallel branches
            run(nhwc_g, tiles_g, out_g.view(N, C, H, W))
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    assert guards_intact(buf_g, img.size)
    assert np.array_equal(bits(tiles_g.cpu().numpy()), bits(want_tiles))
    assert np.array_equal(bits(out_g.cpu().numpy().reshape(N, C, H, W)), bits(eager))


# ---- end to end ---------------------------------------------------------------------------------------------------
S64 = 64


def make_nets(dtype="fp32", S=S64):
    V.configure_seed(42)
    e = V.Encoder([3, S, S], 100, dtype=dtype)
    g = V.Generator(nz=100, img_size=S, dtype=dtype)
    g.apply(V.weights_init)
    e.to(DEV), g.to(DEV)
    return e, g


@pytest.fixture(scope="module")
def nets():
    return make_nets()


def image(N, H, W, seed):
    gen = torch.Generator().manual_seed(seed)
    return (torch.rand(N, 3, H, W, generator=gen) * 2 - 1).to(DEV)


def normal(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def test_denoise_tiled_equals_the_loop_from_public_pieces(nets):
    """3 x 101 x 80, stride 48: 2 x 2 tiles, batch=3 -> chunks of 3 + 1.  The loop: crop each chunk in torch,
    denoise_eval(noisy=chunk, eps_z=...)["recon"], blend with the restatement.  Same chunk sizes -> the tiles are the same
    bits, so against the f32 restatement the result is bit for bit; against the f64 one within the counted bound
    (covers 2 + 2, k = 3: 7 * 2^-24 = 4.17e-7 with |r| <= 1).  Measured on the MI355X: 2.1e-9 (the tiles of the untrained
    networks are of order 1e-3)."""
    e, g = nets
    H, W = 101, 80
    p = R.plan(H, W, S64, 48, "hann")
    assert (p.ny, p.nx) == (2, 2) and p.oy.tolist() == [0, 37] and p.ox.tolist() == [0, 16]
    img = image(1, H, W, 1)
    eps_z = normal((4, 100), 2)
    got = V.denoise_tiled(e, g, img, stride=48, batch=3, eps_z=eps_z)
    assert not e.training and not g.training                               # eval mode, as validation_epoch
    crops = torch.stack([img[0, :, y0:y0 + S64, x0:x0 + S64] for y0 in p.oy for x0 in p.ox]).contiguous()
    recon = torch.cat([V.denoise_eval(e, g, crops[a:b], noisy=crops[a:b], eps_z=eps_z[a:b])["recon"] for a, b in ((0, 3), (3, 4))])
    tiles = recon.cpu().numpy()
    assert got.shape == (1, 3, H, W) and got.dtype == torch.float32
    err = np.abs(got.cpu().numpy().astype(np.float64) - R.blend_f64(p, tiles)).max()
    print("end to end vs the f64 blend of the loop's tiles: max error", err, "bound", R.blend_bound(p, 1.0))
    assert err <= R.blend_bound(p, 1.0)
    assert np.array_equal(bits(got.cpu().numpy()), bits(R.blend_f32(p, tiles)))


def test_one_tile_equals_denoise_eval_bit_for_bit(nets):
    e, g = nets
    e.eval(), g.eval()
    img, eps_z = image(3, S64, S64, 4), normal((3, 100), 5)
    want = V.denoise_eval(e, g, img, noisy=img, eps_z=eps_z)["recon"]
    got = V.denoise_tiled(e, g, img, eps_z=eps_z)
    assert torch.equal(got, want)


def test_sample_false_is_zero_eps_and_sampling_draws_per_tile(nets):
    e, g = nets
    img = image(1, 101, 80, 6)
    a = V.denoise_tiled(e, g, img, stride=48, sample=False)
    b = V.denoise_tiled(e, g, img, stride=48, eps_z=torch.zeros(4, 100, device=DEV))
    assert torch.equal(a, b)
    V.configure_seed(9)
    c = V.denoise_tiled(e, g, img, stride=48)
    V.configure_seed(9)
    d = V.denoise_tiled(e, g, img, stride=48)
    assert torch.equal(c, d) and not torch.equal(c, a) and bool(torch.isfinite(c).all())


def test_resident_u8_source_equals_the_normalised_f32_source(nets):
    e, g = nets
    u8 = torch.randint(0, 256, (2, 80, 101, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(8))
    res = V.ResidentImages(u8, DEV)
    f32 = res.batch(torch.arange(2, device=DEV))
    eps_z = normal((8, 100), 10)
    want = V.denoise_tiled(e, g, f32, stride=48, eps_z=eps_z, batch=5)
    assert torch.equal(V.denoise_tiled(e, g, res, stride=48, eps_z=eps_z, batch=5), want)
    want1 = V.denoise_tiled(e, g, f32[1:], stride=48, eps_z=eps_z[4:], batch=4)
    assert torch.equal(V.denoise_tiled(e, g, res.images[1:], stride=48, eps_z=eps_z[4:], batch=4), want1)   # a slice of the set


def test_tiled_denoise_eval_numbers_are_those_of_the_existing_kernels(nets):
    e, g = nets
    img, eps = image(2, 80, 101, 12), normal((2, 3, 80, 101), 13)
    out = V.tiled_denoise_eval(e, g, img, sigma=0.1, eps=eps, stride=48, sample=False)
    noisy, recon = out["noisy"], out["recon"]
    # the noise is added once, to the whole image (the existing kernel; its multiply-add may be fused: one ulp below 2)
    assert float((noisy - (img + 0.1 * eps).clamp(-1, 1)).abs().max()) <= 2.0 ** -23
    assert torch.equal(recon, V.denoise_tiled(e, g, noisy, stride=48, sample=False)) and out["tiles"] == 8
    scal = torch.zeros(2, device=DEV)
    ops.mse_forward_backward(recon, img, 1.0, scal[0:1], False)
    ops.mse_forward_backward(noisy, img, 1.0, scal[1:2], False)
    mse_r, mse_n = scal.tolist()
    assert out["recon_loss"] == mse_r and out["noisy_loss"] == mse_n
    assert out["ssim"] == float(ops.ssim(recon, img).item()) and out["ssim_noisy"] == float(ops.ssim(noisy, img).item())
    assert abs(out["psnr"] - 10.0 * np.log10(4.0 / mse_r)) < 1e-9
    assert abs(out["psnr_noisy"] - 10.0 * np.log10(4.0 / mse_n)) < 1e-9
    assert out["psnr_noisy"] > 20.0 and 0.0 < out["ssim_noisy"] < 1.0
    given = V.tiled_denoise_eval(e, g, img, noisy=noisy, stride=48, sample=False)
    assert given["noisy"] is not None and torch.equal(given["recon"], recon) and given["recon_loss"] == mse_r


def test_tiled_test_epoch_numbers_are_those_of_the_existing_kernels(nets):
    """Two batches of 1 and 2 images.  The pass accumulates b * metric per batch in f32 on the device: one product and one sum
    rounded per batch and metric, 4 roundings of 2^-24 relative at most -> 1e-6 relative is asserted."""
    e, g = nets
    clean = [image(1, 80, 101, 20), image(2, 80, 101, 21)]
    noisy = [(c + 0.1 * normal(tuple(c.shape), 22 + i)).clamp(-1, 1) for i, c in enumerate(clean)]
    out = V.tiled_test_epoch(e, g, zip(noisy, clean), stride=48, sample=False)
    sums = np.zeros(4)
    for n_, c_ in zip(noisy, clean):
        r_ = V.denoise_tiled(e, g, n_, stride=48, sample=False)
        scal = torch.zeros(2, device=DEV)
        ops.mse_forward_backward(r_, c_, 1.0, scal[0:1], False)
        ops.mse_forward_backward(n_, c_, 1.0, scal[1:2], False)
        m = scal.tolist()
        sums += c_.shape[0] * np.array([m[0], float(ops.ssim(r_, c_).item()), m[1], float(ops.ssim(n_, c_).item())])
    mse_r, ssim_r, mse_n, ssim_n = sums / 3
    assert (out["samples"], out["tiles"]) == (3, 12)
    assert set(out) == {"psnr", "ssim", "recon_loss", "psnr_noisy", "ssim_noisy", "samples", "tiles"}
    for got, want in ((out["recon_loss"], mse_r), (out["ssim"], ssim_r), (out["ssim_noisy"], ssim_n)):
        assert abs(got - want) <= 1e-6 * abs(want), (got, want)
    assert abs(out["psnr"] - 10 * np.log10(4 / mse_r)) < 1e-4 and abs(out["psnr_noisy"] - 10 * np.log10(4 / mse_n)) < 1e-4
    with pytest.raises(RuntimeError, match="no batch"):
        V.tiled_test_epoch(e, g, [])


def test_bf16_engines_run_and_stay_in_range():
    e, g = make_nets("bf16")
    img = image(2, 101, 80, 30)
    out = V.denoise_tiled(e, g, img, stride=48, batch=128)
    assert out.shape == (2, 3, 101, 80) and bool(torch.isfinite(out).all()) and float(out.abs().max()) <= 1.0
    u8 = torch.randint(0, 256, (1, 70, 90, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(31)).to(DEV)
    out = V.denoise_tiled(e, g, u8, window="tri", sample=False)
    assert out.shape == (1, 3, 70, 90) and bool(torch.isfinite(out).all()) and float(out.abs().max()) <= 1.0


def test_denoise_tiled_at_s128_equals_the_loop_from_public_pieces():
    """The twin of the S = 64 test with the S = 128 engines (gather grid.z 2): 3 x 150 x 203, default stride 64: 2 x 3 tiles,
    x origins 0, 64, 75 (the flush one odd), batch=4 -> chunks of 4 + 2.  Bit for bit against the f32 restatement of the loop's
    tiles; against the f64 one within the counted bound (covers 2 + 3, k = 3: 8 * 2^-24 = 4.77e-7 with |r| <= 1).
    Measured on the MI355X: 3.8e-10, error / bound 7.9e-4 (the tiles of the untrained networks are below 4e-3).  S = 256 end to end is left out (two more engines to build for a blend and a gather
    whose grids the kernel-level cases above already reach)."""
    S, H, W = 128, 150, 203
    e, g = make_nets(S=S)
    p = R.plan(H, W, S)
    assert (p.ny, p.nx) == (2, 3) and p.oy.tolist() == [0, 22] and p.ox.tolist() == [0, 64, 75] and p.stride == 64
    img = image(1, H, W, 40)
    eps_z = normal((6, 100), 41)
    got = V.denoise_tiled(e, g, img, batch=4, eps_z=eps_z)
    assert not e.training and not g.training
    crops = torch.stack([img[0, :, y0:y0 + S, x0:x0 + S] for y0 in p.oy for x0 in p.ox]).contiguous()
    recon = torch.cat([V.denoise_eval(e, g, crops[a:b], noisy=crops[a:b], eps_z=eps_z[a:b])["recon"] for a, b in ((0, 4), (4, 6))])
    tiles = recon.cpu().numpy()
    assert got.shape == (1, 3, H, W) and got.dtype == torch.float32
    err = np.abs(got.cpu().numpy().astype(np.float64) - R.blend_f64(p, tiles)).max()
    print("S = 128 end to end vs the f64 blend of the loop's tiles: max error", err, "bound", R.blend_bound(p, 1.0),
          "ratio", err / R.blend_bound(p, 1.0), "max|tile|", float(np.abs(tiles).max()))
    assert float(np.abs(tiles).max()) <= 1.0 and err <= R.blend_bound(p, 1.0)
    assert np.array_equal(bits(got.cpu().numpy()), bits(R.blend_f32_fast(p, tiles)))


def test_bf16_engines_at_s128_run_and_stay_in_range():
    e, g = make_nets("bf16", S=128)
    out = V.denoise_tiled(e, g, image(1, 150, 203, 42), batch=4)
    assert out.shape == (1, 3, 150, 203) and bool(torch.isfinite(out).all()) and float(out.abs().max()) <= 1.0


def test_refused_inputs_raise(nets):
    e, g = nets
    for shape, kw in (((1, 3, 63, 80), {}), ((1, 3, 80, 63), {}), ((1, 3, 80, 80), dict(stride=0)), ((1, 3, 80, 80), dict(stride=65)),
                      ((1, 3, 137, 64), dict(stride=8)),                   # 9 tiles would cover row 73: above VG_TILE_MAX_COVER
                      ((1, 3, 80, 80), dict(window="gauss")), ((1, 3, 80, 80), dict(batch=0)),
                      ((1, 3, 80, 80), dict(eps_z=torch.zeros(3, 100, device=DEV))),
                      ((1, 3, 80, 80), dict(eps_z=torch.zeros(4, 100))), ((1, 1, 80, 80), {})):
        with pytest.raises(RuntimeError):
            V.denoise_tiled(e, g, torch.zeros(*shape, device=DEV), **kw)
    with pytest.raises(RuntimeError):
        V.denoise_tiled(e, g, torch.zeros(1, 3, 80, 80, dtype=torch.float64, device=DEV))
    with pytest.raises(RuntimeError):
        V.tiled_denoise_eval(e, g, torch.zeros(1, 3, 80, 80, device=DEV), noisy=torch.zeros(1, 3, 80, 81, device=DEV))
    plan = T.tile_plan(20, 12, 8, 4)
    with pytest.raises(RuntimeError):
        ops.tile_gather(torch.zeros(1, 3, 20, 16, device=DEV), plan, 0, 1, 4, G.F32)          # not the plan's image size
    with pytest.raises(RuntimeError):
        ops.tile_gather(torch.zeros(1, 3, 20, 12, device=DEV), plan, 7, 2, 4, G.F32)          # t0 + B past the 8 tiles
    with pytest.raises(RuntimeError):
        ops.tile_blend(torch.zeros(7, 3, 8, 8, device=DEV), plan)                             # not a whole number of images
