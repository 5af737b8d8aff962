"""GPU: the degraded-pair data path (vg_gather_degrade_u8 and the layers above it) against a plain restatement of
CelebADatasetV0.add_noise (dataset_code.py:35-56) fed with the MATERIALISED draws.  Device draws can never equal torch's
CPU generator, so parity is "kernel == restatement on the draws vg_randn / vg_rand_u01 hand out", bit for bit, plus
distribution checks of the per-image parameters.  Every expectation is derived from the materialisers and the contract
text in include/vaegan_hip.h ("Degraded pairs"), never from the kernel under test."""
import math

import pytest
import torch

import vaegan_amd as V
from test_gpu_data import jpeg_folder  # noqa: F401  (fixture: 45 generated 64 x 64 JPEGs)
from test_gpu_parity import build

pytestmark = pytest.mark.gpu
DEV = "cuda"
ops, data, G = V.ops, V.data, V.geometry
DRAW_N, DRAW_FILL, DRAW_PARAMS = 16, 17, 18            # the header's VG_DRAW_DEGRADE_NORMAL / _FILL / _PARAMS


# ---- the restatement -------------------------------------------------------------------------------------------------
def add_noise_ref(clean, n, fill, s, noise_max_std, rect, rect_h, rect_w, x, y):
    """clean, n, fill: [C,H,W] f32 on the host.  Rectangle first (replaced by 2*fill - 1 at the pixel's own index), then
    + (n * s) * noise_max_std with one s per image, then clamp."""
    img = clean.clone()
    if rect:
        img[:, y:y + rect_h, x:x + rect_w] = fill[:, y:y + rect_h, x:x + rect_w] * 2.0 - 1.0
    noise = n * torch.tensor(s, dtype=torch.float32) * noise_max_std
    return torch.clamp(img + noise, -1.0, 1.0)


def state_at(seed, pos):
    return torch.tensor([seed, pos], dtype=torch.int64, device=DEV)


def randn_at(seed, pos, n, draw):
    ns = ops.NoiseStream(DEV, seed)
    ns.state.copy_(state_at(seed, pos))
    return ns.randn((n,), draw)


def params_from_words(seed, pos, rect, bounds):
    """s, rect_h, rect_w, x, y by the header's formulas from the words behind vg_rand_u01(draw PARAMS): u = k * 2^-24
    with k = word >> 8, rint(lo, hi) = lo + ((k * (hi - lo)) >> 24)."""
    u = ops.rand_u01(8, state_at(seed, pos), DRAW_PARAMS).cpu()
    k = [int(round(float(v) * 2 ** 24)) for v in u]
    assert all(float(v) == kk * 2.0 ** -24 for v, kk in zip(u, k))
    s = float(u[0])
    if not rect:
        return s, 0, 0, 0, 0

    def rint(kk, lo, hi):
        return lo + ((kk * (hi - lo)) >> 24)
    lo, hi, x0, x1, y0, y1 = bounds
    rect_h, rect_w = rint(k[1], lo, hi + 1), rint(k[2], lo, hi + 1)
    return s, rect_h, rect_w, rint(k[3], x0, x1 - rect_w), rint(k[4], y0, y1 - rect_h)


# ---- 4: exactness ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("rect", [True, False])
@pytest.mark.parametrize("shape", [(64, 64, 3), (50, 50, 3), (32, 48, 1)])
def test_pairs_equal_the_restatement_on_the_materialised_draws_bitwise(shape, rect, normalize):
    H, W, C = shape
    B, pos0, nms, N = 37, 1000, 0.3, 9          # 0.3: not a power of two, so a contracted multiply-add would show
    gen = torch.Generator().manual_seed(H * 1000 + W + C)
    images = torch.randint(0, 256, (N, H, W, C), dtype=torch.uint8, generator=gen)
    images[0, :4] = 0
    images[0, 4:8] = 255                                                   # the extreme bytes are present
    idx = torch.randint(0, N, (B,), generator=gen)                        # 37 draws from 9 images: repeated indices
    assert idx.unique().numel() < B
    dimg, didx = images.to(DEV), idx.to(DEV)
    bounds = data.degrade_bounds(H, W)
    u255 = images.permute(0, 3, 1, 2).to(torch.float32).div(255)
    for seed in (20240607, 3):
        noisy, clean, _ = ops.gather_degrade_u8(dimg, didx, seed, pos0, nms, rect, normalize, bounds)
        CP = G.padc(C, G.BF16)
        nhwc = {dt: ops.gather_degrade_u8(dimg, didx, seed, pos0, nms, rect, normalize, bounds, nhwc=(CP, dt))
                for dt in (G.F32, G.BF16)}
        got_params = ops.degrade_params(seed, pos0, B, nms, rect, H, W, bounds).cpu()
        if normalize:
            want_clean = ops.gather_normalize_u8(dimg, didx).cpu()
            assert torch.equal(want_clean, u255[idx].sub(0.5).div(0.5))
        else:
            want_clean = u255[idx]
        assert torch.equal(clean.cpu(), want_clean)
        want, sizes = [], []
        for b in range(B):
            pos = pos0 + b
            n = randn_at(seed, pos, C * H * W, DRAW_N).cpu().view(C, H, W)
            fill = ops.rand_u01(C * H * W, state_at(seed, pos), DRAW_FILL).cpu().view(C, H, W)
            s, rh, rw, x, y = params_from_words(seed, pos, rect, bounds)
            want.append(add_noise_ref(want_clean[b], n, fill, s, nms, rect, rh, rw, x, y))
            sizes.append((rh, rw))
            exp = torch.tensor([s, 0.0, rh, rw, x, y, 0, 0], dtype=torch.float32)
            exp[1] = torch.tensor(s, dtype=torch.float32) * nms
            assert torch.equal(got_params[b], exp), (b, got_params[b], exp)
        want = torch.stack(want)
        assert torch.equal(noisy.cpu(), want)
        if rect:
            assert any(rh > 0 and rw > 0 for rh, rw in sizes)
        for dt, (n2, c2, y) in nhwc.items():
            assert torch.equal(n2, noisy) and torch.equal(c2, clean)
            assert y.shape == (B, H, W, CP) and torch.equal(y, ops.nchw_to_nhwc(noisy, CP, dt))
    # different seeds give different noise
    a = ops.gather_degrade_u8(dimg, didx, 20240607, pos0, nms, rect, normalize, bounds)[0]
    assert not torch.equal(a, noisy)


# ---- 5: the uniform materialiser -------------------------------------------------------------------------------------
def test_rand_u01_grid_and_prefix_property():
    st = state_at(77, 5)
    u = ops.rand_u01(100003, st, DRAW_FILL).cpu().double()
    k = u * 2 ** 24
    assert torch.equal(k, k.round()) and float(k.min()) >= 0 and float(k.max()) < 2 ** 24
    assert abs(float(u.mean()) - 0.5) < 5 / math.sqrt(12 * u.numel())
    for n in (1, 2, 3, 4, 5, 1023, 4099):
        assert torch.equal(ops.rand_u01(n, st, DRAW_FILL).cpu().double(), u[:n])
    assert not torch.equal(ops.rand_u01(4099, st, DRAW_PARAMS).cpu().double(), u[:4099])       # another draw id
    assert not torch.equal(ops.rand_u01(4099, state_at(77, 6), DRAW_FILL).cpu().double(), u[:4099])


# ---- 6: keying ---------------------------------------------------------------------------------------------------------
def test_degradation_is_keyed_by_seed_and_epoch_position_not_by_batch_slot():
    H = W = 64
    gen = torch.Generator().manual_seed(8)
    images = torch.randint(0, 256, (6, H, W, 3), dtype=torch.uint8, generator=gen).to(DEV)
    bounds = data.degrade_bounds(H, W)
    idx = torch.tensor([5, 1, 4, 2, 0, 3, 2], device=DEV)
    n1, c1, _ = ops.gather_degrade_u8(images, idx, 99, 40, 0.25, True, True, bounds)
    n2, c2, _ = ops.gather_degrade_u8(images, idx[3:5].contiguous(), 99, 43, 0.25, True, True, bounds)
    assert torch.equal(n1[3:5], n2) and torch.equal(c1[3:5], c2)          # slot 3 of one call == slot 0 of the other
    n3 = ops.gather_degrade_u8(images, idx[3:5].contiguous(), 99, 44, 0.25, True, True, bounds)[0]
    n4 = ops.gather_degrade_u8(images, idx[3:5].contiguous(), 100, 43, 0.25, True, True, bounds)[0]
    assert not torch.equal(n3, n2) and not torch.equal(n4, n2)
    assert not torch.equal(n1[3], n1[6])                                   # the same image at two positions
    with pytest.raises(RuntimeError):
        ops.gather_degrade_u8(images, idx, -1, 0, 0.25, True, True, bounds)
    with pytest.raises(RuntimeError):
        ops.gather_degrade_u8(images, idx, 1, 0, 0.25, True, True, None)   # rect without bounds


# ---- 7: distribution -----------------------------------------------------------------------------------------------------
def test_distribution_of_the_per_image_parameters_over_4096_positions():
    H = W = 64
    P, nms, seed, chunk = 4096, 0.25, 424242, 256
    gen = torch.Generator().manual_seed(9)
    images = torch.randint(0, 256, (64, H, W, 3), dtype=torch.uint8, generator=gen).to(DEV)
    bounds = data.degrade_bounds(H, W)
    assert bounds == (1, 16, 16, 49, 16, 49)
    prm = ops.degrade_params(seed, 0, P, nms, True, H, W, bounds).cpu().double()
    s, rh, rw, x, y = prm[:, 0], prm[:, 2].long(), prm[:, 3].long(), prm[:, 4].long(), prm[:, 5].long()
    assert int(rh.min()) >= 1 and int(rh.max()) <= 16 and int(rw.min()) >= 1 and int(rw.max()) <= 16
    assert bool((x >= 16).all()) and bool((x < 49 - rw).all()) and bool((y >= 16).all()) and bool((y < 49 - rh).all())
    assert bool((x + rw <= 48).all()) and bool((y + rh <= 48).all())      # the rectangle lies inside [16, 49)^2
    assert sorted(rh.unique().tolist()) == list(range(1, 17)) == sorted(rw.unique().tolist())
    se_rect = math.sqrt((16 ** 2 - 1) / 12 / P)
    print(f"mean rect_h {float(rh.double().mean()):.4f} rect_w {float(rw.double().mean()):.4f} (8.5 +- {5 * se_rect:.3f}); "
          f"mean s {float(s.mean()):.5f} (0.5 +- {5 / math.sqrt(12 * P):.4f})")
    assert abs(float(rh.double().mean()) - 8.5) <= 5 * se_rect and abs(float(rw.double().mean()) - 8.5) <= 5 * se_rect
    assert float(s.min()) >= 0 and float(s.max()) < 1 and abs(float(s.mean()) - 0.5) <= 5 / math.sqrt(12 * P)
    hh = torch.arange(H, device=DEV).view(1, 1, H, 1)
    ww = torch.arange(W, device=DEV).view(1, 1, 1, W)
    fill_sum, fill_cnt, clamped, total = 0.0, 0, 0, 0
    for p0 in range(0, P, chunk):
        idx = (torch.arange(p0, p0 + chunk, device=DEV) * 7) % 64
        noisy, clean, _ = ops.gather_degrade_u8(images, idx, seed, p0, nms, True, True, bounds)
        assert float(noisy.abs().max()) <= 1.0
        fill = torch.empty(chunk, 3 * H * W, dtype=torch.float32, device=DEV)
        for b in range(chunk):
            ops.rand_u01(3 * H * W, state_at(seed, p0 + b), DRAW_FILL, out=fill[b])
        g = prm[p0:p0 + chunk].to(DEV)
        gy, gx = g[:, 5].view(-1, 1, 1, 1), g[:, 4].view(-1, 1, 1, 1)
        mask = (hh >= gy) & (hh < gy + g[:, 2].view(-1, 1, 1, 1)) & (ww >= gx) & (ww < gx + g[:, 3].view(-1, 1, 1, 1))
        mask = mask.expand(chunk, 3, H, W)
        vals = (fill.view(chunk, 3, H, W).double() * 2 - 1)[mask]
        fill_sum += float(vals.sum())
        fill_cnt += int(mask.sum())
        clamped += int((noisy.abs() == 1.0).sum())
        total += noisy.numel()
        # outside the rectangle the clean image shows through wherever the sum was not clamped
        free = ~mask & (noisy.abs() < 1.0)
        sig = g[:, 1].view(-1, 1, 1, 1).float()
        # |n| <= sqrt(-2 ln 2^-33) = 6.77 (Box-Muller on u >= 2^-33); 2.4e-7 = two ulps at 1: the rounded sum (half an ulp
        # at 1) and this subtraction (half an ulp at 2)
        assert bool(((noisy - clean).abs()[free] <= 6.8 * sig.expand_as(noisy)[free] + 2.4e-7).all())
    assert fill_cnt == int((rh * rw).sum()) * 3
    se_fill = math.sqrt(1.0 / 3.0 / fill_cnt)
    print(f"fill mean {fill_sum / fill_cnt:+.6f} over {fill_cnt} rectangle elements (0 +- {5 * se_fill:.6f}); "
          f"clamped share {clamped / total:.4f}")
    assert abs(fill_sum / fill_cnt) <= 5 * se_fill


# ---- 8 - 10: loaders -------------------------------------------------------------------------------------------------
def test_degraded_loader_clean_halves_equal_the_plain_loader_and_noise_follows_the_seed(jpeg_folder):  # noqa: F811
    ds = data.ResidentImages.from_folder(jpeg_folder, device=DEV, workers=1)
    idx = torch.arange(len(ds))
    torch.manual_seed(42)
    plain_loader = data.DeviceLoader(ds, idx, 8, shuffle=True)
    plain = [[b.cpu() for b in plain_loader] for _ in range(2)]
    runs = []
    for _ in range(2):
        torch.manual_seed(42)
        loader = data.DeviceLoader(ds, idx, 8, shuffle=True, degrade=data.Degrade(0.25))
        epochs, seeds = [], []
        for _ in range(2):
            epochs.append([(n.cpu(), c.cpu()) for n, c in loader])
            seeds.append(loader.last_base_seed)
        runs.append((epochs, seeds))
    (epochs, seeds), (epochs2, seeds2) = runs
    assert seeds == seeds2 and seeds[0] != seeds[1]
    for e in range(2):
        assert len(epochs[e]) == len(plain[e]) == 6 and epochs[e][-1][1].shape[0] == 5          # 45 = 5 * 8 + 5
        for (n, c), p, (n2, c2) in zip(epochs[e], plain[e], epochs2[e]):
            assert torch.equal(c, p) and torch.equal(n, n2) and torch.equal(c, c2)
            assert n.shape == c.shape and float(n.abs().max()) <= 1.0 and not torch.equal(n, c)
    # epoch 1's noise is not epoch 0's: compare the residual on the same image (index 0 of the set) in both epochs
    loader = data.DeviceLoader(ds, idx, 45, shuffle=False, degrade=data.Degrade(0.25, rect=False))
    torch.manual_seed(1)
    (n0, c0), = list(loader)
    (n1, c1), = list(loader)
    assert torch.equal(c0, c1) and not torch.equal(n0, n1)


def test_two_rank_degraded_shards_concatenate_to_the_single_process_batches(jpeg_folder):  # noqa: F811
    ds = data.ResidentImages.from_folder(jpeg_folder, device=DEV, workers=1)
    idx = torch.arange(len(ds))
    dg = data.Degrade(0.25)
    torch.manual_seed(3)
    whole = [(n.cpu(), c.cpu()) for n, c in data.DeviceLoader(ds, idx, 16, shuffle=True, degrade=dg)]
    parts = []
    for r in range(2):
        torch.manual_seed(3)
        parts.append([(n.cpu(), c.cpu()) for n, c in data.DeviceLoader(ds, idx, 8, shuffle=True, rank=r, world=2, degrade=dg)])
    assert len(parts[0]) == len(parts[1]) == len(whole) == 3
    for k, w in enumerate(whole):
        for half in (0, 1):
            both = torch.cat([parts[0][k][half], parts[1][k][half]])
            assert torch.equal(both, w[half][:both.shape[0]])
            assert w[half].shape[0] - both.shape[0] < 2
    assert whole[-1][0].shape[0] == 13 and parts[0][-1][0].shape[0] == 6


def test_get_dataset_loaders_lq_pairs_and_unchanged_defaults(jpeg_folder):  # noqa: F811
    torch.manual_seed(42)
    tl, vl, shape = data.get_dataset_loaders(jpeg_folder, batch_size=8, device=DEV, workers=1, dataset_type="LQ",
                                             image_size=(32, 32), noise_max_std=0.25)
    assert tuple(shape) == (3, 32, 32)
    seen = 0
    for loader in (tl, vl):
        for noisy, clean in loader:
            assert noisy.shape == clean.shape and tuple(clean.shape[1:]) == (3, 32, 32) and clean.dtype == torch.float32
            assert float(clean.min()) >= 0.0 and float(clean.max()) <= 1.0 and float(clean.max()) > 0.5
            assert float(noisy.min()) >= -1.0 and float(noisy.max()) <= 1.0
            seen += clean.shape[0]
    assert seen == 45
    # 'LQ' without noise: clean batches in V0's value range
    torch.manual_seed(42)
    tl2, _, _ = data.get_dataset_loaders(jpeg_folder, batch_size=8, device=DEV, workers=1, dataset_type="LQ", image_size=(32, 32))
    plain = list(tl2)                                                    # split + epoch order drawn back to back ...
    torch.manual_seed(42)
    tl3, _, _ = data.get_dataset_loaders(jpeg_folder, batch_size=8, device=DEV, workers=1, dataset_type="LQ",
                                         image_size=(32, 32), noise_max_std=0.25)
    paired = list(tl3)                                                   # ... from the same seed for both loaders
    assert len(plain) == len(paired) == 5                                # 40 training images
    for b, (_, c) in zip(plain, paired):
        assert torch.is_tensor(b) and torch.equal(b, c)
    # defaults: exactly the plain 'HQ' loaders (a restatement of what the function did before it grew the arguments)
    torch.manual_seed(42)
    tl, vl, shape = data.get_dataset_loaders(jpeg_folder, batch_size=8, device=DEV, workers=1)
    got = [[b.cpu() for b in tl], [b.cpu() for b in vl]]
    torch.manual_seed(42)
    ds = data.ResidentImages.from_folder(jpeg_folder, None, DEV, 1)
    tr_idx, te_idx = data.random_split_indices(len(ds), 0.9)
    want = [[b.cpu() for b in data.DeviceLoader(ds, tr_idx, 8, shuffle=True)],
            [b.cpu() for b in data.DeviceLoader(ds, te_idx, 8, shuffle=False)]]
    assert tuple(shape) == (3, 64, 64) and tl.degrade is None and vl.degrade is None
    for a, b in zip(got, want):
        assert len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b))


# ---- 11: the paired test pass ------------------------------------------------------------------------------------------
def test_paired_test_epoch_vs_cpu_restatement_on_the_oracle_nets(jpeg_folder):  # noqa: F811
    """main_vae.py:251-266 on the oracle's nets (weights synced as the validation-epoch test does), injected eps_z, the
    device-made pairs copied to the host as the restatement's input.  The restatement clamps logvar to [-10, 10] as the
    engine does (documented deviation; inert here)."""
    import vaegan_ref as R
    from _inputs import make_inputs
    from test_gpu_parity import sync_from_oracle
    S = 64
    ds = data.ResidentImages.from_folder(jpeg_folder, device=DEV, workers=1)
    loader = data.DeviceLoader(ds, torch.arange(40, 45), 2, shuffle=False, degrade=data.Degrade(0.25))
    torch.manual_seed(5)
    pairs = [(n.cpu(), c.cpu()) for n, c in loader]                            # 5 images: 2 + 2 + 1
    e, g, d, tr = build(S)
    o = R.RefVAEGAN(img_size=S, seed=42)
    real, ez, er, ec = make_inputs(4, S, 4711)
    o.train_step(real, ez, er, ec, 60)                                         # non-trivial BatchNorm running statistics
    sync_from_oracle(o, e, g, d, tr)
    gen = torch.Generator().manual_seed(99)
    eps = [torch.randn(c.shape[0], 100, generator=gen) for _, c in pairs]
    tot, seen, ssim_r, ssim_n, se_r, se_n = 0.0, 0, 0.0, 0.0, 0.0, 0.0
    with torch.no_grad():
        for (noisy, clean), eps_z in zip(pairs, eps):
            mu, logvar = R.encoder_forward(o.E, noisy, False)
            logvar = torch.clamp(logvar, min=-10, max=10)
            z = (mu + torch.exp(0.5 * logvar) * eps_z).unsqueeze(-1).unsqueeze(-1)
            recon = R.generator_forward(o.G, o.g_spec, z, False)
            tot += float(torch.nn.functional.mse_loss(recon, clean, reduction="sum") + R.kl_sum(mu, logvar))
            b = clean.shape[0]
            c01 = (clean + 1) / 2
            ssim_r += R.ssim((recon + 1) / 2, c01) * b
            ssim_n += R.ssim((noisy + 1) / 2, c01) * b
            se_r += float((((recon + 1) / 2).double() - c01.double()).pow(2).mean()) * b
            se_n += float((((noisy + 1) / 2).double() - c01.double()).pow(2).mean()) * b
            seen += b
    want = {"test_loss": tot / seen, "ssim": ssim_r / seen, "ssim_noisy": ssim_n / seen,
            "psnr": 10 * math.log10(1 / (se_r / seen)), "psnr_noisy": 10 * math.log10(1 / (se_n / seen))}
    torch.manual_seed(5)                                                        # the same epoch seed -> the same pairs
    got = V.paired_test_epoch(e, g, loader, noise_fn=lambda i, noisy: eps[i].to(DEV))
    print("paired_test_epoch", got, "restatement", want)
    assert not e.training and not g.training and got["samples"] == 5 and got["batches"] == 3
    assert loader._nhwc is None                                                 # the NHWC request is withdrawn afterwards
    assert abs(got["test_loss"] - want["test_loss"]) <= 1e-4 * abs(want["test_loss"])
    assert abs(got["ssim"] - want["ssim"]) < 1e-4 and abs(got["ssim_noisy"] - want["ssim_noisy"]) < 1e-4
    assert abs(got["psnr"] - want["psnr"]) < 1e-3 and abs(got["psnr_noisy"] - want["psnr_noisy"]) < 1e-3
    # a plain iterable of pairs (no NHWC offer) gives the same numbers: the loader's NHWC copy == the separate pass
    again = V.paired_test_epoch(e, g, [(n.to(DEV), c.to(DEV)) for n, c in pairs], noise_fn=lambda i, noisy: eps[i].to(DEV))
    assert again == got


# ---- 12: wiring --------------------------------------------------------------------------------------------------------
def test_training_on_the_clean_half_and_denoise_eval_on_the_noisy_half_run(jpeg_folder):  # noqa: F811
    torch.manual_seed(42)
    tl, vl, shape = data.get_dataset_loaders(jpeg_folder, batch_size=16, device=DEV, workers=1, noise_max_std=0.25)
    e, g, d, tr = build(shape[1])
    losses = []
    for noisy, clean in tl:
        losses.append(tr.train_step(clean, 60)[:5].clone())
    torch.cuda.synchronize()
    assert len(losses) == 3 and all(bool(torch.isfinite(l).all()) for l in losses)
    e.eval(), g.eval()
    noisy, clean = next(iter(vl))
    out = V.denoise_eval(e, g, clean, noisy=noisy)
    assert torch.equal(out["noisy"], noisy) and out["recon"].shape == clean.shape
    assert all(math.isfinite(out[k]) for k in ("recon_loss", "kl_loss", "val_loss", "psnr", "ssim"))
