"""GPU: tiled denoising (vg_tile_gather, vg_tile_blend, and denoise_tiled / tiled_denoise_eval / tiled_test_epoch above them)
against the numpy restatement tests/_tiling_ref.py.  The gather and the exact-input blends (tests/test_tiling_cpu.py shows
that every product and partial sum of theirs is an f32 number) are compared bit for bit; random inputs within the bound
counted from the roundings (_tiling_ref.blend_bound).  No expectation is taken from the kernel under test.  Every kernel
output is a NaN-filled slice of a larger NaN-filled buffer: a stale right answer in recycled memory cannot pass, and a store
before or past the output shows in the guard rows."""
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


# ---- end to end ---------------------------------------------------------------------------------------------------
S64 = 64


def make_nets(dtype="fp32"):
    V.configure_seed(42)
    e = V.Encoder([3, S64, S64], 100, dtype=dtype)
    g = V.Generator(nz=100, img_size=S64, dtype=dtype)
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
