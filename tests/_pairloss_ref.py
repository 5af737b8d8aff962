"""Test infrastructure for training on degraded pairs, CPU only:

  region_mask / region_mse / region_mse_grad   f64 restatement of the contract of vg_region_mse_forward_backward
                                               (include/vaegan_hip.h), evaluated on the f32 inputs;
  ref_step / ref_vae_step                      oracle/vaegan_ref.RefVAEGAN.train_step and oracle/siblings_ref.RefVAE.train_step
                                               with the Encoder fed `noisy` and the region-weighted reconstruction term,
                                               written with those modules' own functions (the oracles are imported, not edited);
  ref_paired_regions                           the region metrics of denoise.paired_test_epoch(regions=True);
  cycle_rects / make_noisy                     the rectangles and the degraded inputs the tests use.
"""
import math

import torch

import vaegan_ref as R
from _pointwise_ref import U, f32

NAN = float("nan")


# ---- the kernel contract in f64 --------------------------------------------------------------------------------------
def region_mask(rects, B, C, H, W):
    """-> bool [B, C, H, W]: pixel (h, w) of image i is in the hole iff y <= h < y + rect_h and x <= w < x + rect_w with
    {rect_h, rect_w, x, y} = rects[i][2..5], in every channel; the comparisons (and the two sums) are f32, as the kernel's.
    None: no hole.  A NaN makes every comparison false; a rectangle past the image is clipped by the image."""
    if rects is None:
        return torch.zeros(B, C, H, W, dtype=torch.bool)
    r = rects.detach().cpu().float()
    assert tuple(r.shape) == (B, 8)
    rh, rw, x, y = (r[:, k].view(B, 1, 1) for k in (2, 3, 4, 5))
    h = torch.arange(H, dtype=torch.float32).view(1, H, 1)
    w = torch.arange(W, dtype=torch.float32).view(1, 1, W)
    m = (h >= y) & (h < y + rh) & (w >= x) & (w < x + rw)             # [B, H, W]
    return m.unsqueeze(1).expand(B, C, H, W).clone()


def region_mse(a, b, rects, w_hole):
    """-> (loss, hole_mse, S_hole, S_valid, n_hole, n_valid), all f64 python floats / ints:
    loss = (S_valid + w_hole S_hole) / n, hole_mse = S_hole / n_hole (0 without a hole)."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    m = region_mask(rects, *a.shape)
    q = (a - b) ** 2
    s_hole, s_valid = float(q[m].sum()), float(q[~m].sum())
    n_hole = int(m.sum())
    n = a.numel()
    return ((s_valid + f32(w_hole) * s_hole) / n, s_hole / n_hole if n_hole else 0.0, s_hole, s_valid, n_hole, n - n_hole)


def region_mse_grad(a, b, rects, w_hole, gscale):
    """d (gscale * loss) / d a in f64: 2 gscale (a - b) / n, times w_hole inside the hole."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    m = region_mask(rects, *a.shape)
    coef = torch.where(m, torch.tensor(f32(w_hole), dtype=torch.float64), torch.tensor(1.0, dtype=torch.float64))
    return f32(gscale) * 2.0 * (a - b) * coef / a.numel()


def weighted_mse(recon, target, rects, w_hole):
    """The term as a differentiable torch expression in recon's dtype: -> (L_w, hole_mse)."""
    m = region_mask(rects, *recon.shape)
    mk = m.to(recon.dtype)
    q = (recon - target) ** 2
    l_w = ((mk * w_hole + (1 - mk)) * q).sum() / q.numel()
    n_hole = int(m.sum())
    hole = (mk * q).sum() / n_hole if n_hole else torch.zeros((), dtype=recon.dtype)
    return l_w, hole


# ---- inputs ----------------------------------------------------------------------------------------------------------
def cycle_rects(B, H, W):
    """f32 [B, 8] (s, sigma, rect_h, rect_w, x, y, 0, 0): the batch cycles through the edge cases of the contract."""
    cases = [
        (0, 3, 1, 1),                          # empty by height
        (3, 0, 1, 1),                          # empty by width
        (H, W, 0, 0),                          # the full image
        (1, 1, 0, 0),                          # 1 x 1 at (0, 0)
        (1, 1, W - 1, H - 1),                  # 1 x 1 at (H - 1, W - 1)
        (max(1, H // 3), 3 if W < 12 else 6, 1 if W < 12 else 5, min(1, H - 1)),   # x, rect_w no multiples of 4: hole edges inside a 16-byte vector
        (H, W, W // 2 + 1, H // 2),            # reaching past the right and bottom edges
        (NAN, 5, NAN, 1),                      # a NaN row
    ]
    out = torch.zeros(B, 8)
    for i in range(B):
        rh, rw, x, y = cases[i % len(cases)]
        out[i] = torch.tensor([0.5, 0.1, rh, rw, x, y, 0, 0], dtype=torch.float32)
    return out


def offset_rects(B, H, W, shift):
    """cycle_rects starting at another case, so that small batches meet every case over a few calls."""
    return cycle_rects(B + shift, H, W)[shift:].clone()


def make_noisy(clean, rects, seed, sigma=0.1):
    """A degraded batch made on the host: the rectangles filled uniformly in [-1, 1], plus N(0, sigma^2) noise, clamped."""
    g = torch.Generator().manual_seed(seed)
    m = region_mask(rects, *clean.shape)
    fill = torch.rand(clean.shape, generator=g) * 2 - 1
    noisy = torch.where(m, fill, clean) + sigma * torch.randn(clean.shape, generator=g)
    return noisy.clamp(-1.0, 1.0)


NOISY_SEED = 11         # make_noisy seed of the first-step tests
# make_noisy seed of the isolated gradient-path test, on make_inputs(4, 64, _ssimloss_ref.ISO_SEED) with hand_rects(4): the
# first one from NOISY_SEED on whose fp64 forward keeps every pre-activation at least 2e-6 from zero (2.9e-6; see
# _ssimloss_ref.activation_margin for why; tests/test_pairloss_cpu.py asserts it)
ISO_NOISY_SEED = 37

HAND_RECTS = [(10, 14, 17, 20), (16, 5, 30, 16), (1, 1, 48, 47), (7, 16, 21, 33)]      # rect_h, rect_w, x, y at S = 64


def hand_rects(B):
    out = torch.zeros(B, 8)
    for i in range(B):
        rh, rw, x, y = HAND_RECTS[i % len(HAND_RECTS)]
        out[i] = torch.tensor([0.5, 0.1, rh, rw, x, y, 0, 0], dtype=torch.float32)
    return out


# ---- the iterations --------------------------------------------------------------------------------------------------
def ref_step(model, clean, noisy, eps_z, eps_real, eps_recon, epoch, rects=None, hole_weight=1.0, alpha_kl=0.1, alpha_adv=0.1):
    """RefVAEGAN.train_step (vaegan_code.py:65-135) on a degraded pair: encoder_forward(E, noisy); the Discriminator's real
    batch and the reconstruction target are `clean`; with rects and hole_weight != 1 the reconstruction term is the
    region-weighted MSE L_w ("recon_loss" then holds L_w and the dict gains "hole_mse")."""
    m = model
    B = clean.size(0)
    dt = getattr(m, "dtype", torch.float32)
    clean, noisy, eps_z, eps_real, eps_recon = (t.to(dt) for t in (clean, noisy, eps_z, eps_real, eps_recon))
    mu, logvar = R.encoder_forward(m.E, noisy, True)
    logvar = torch.clamp(logvar, min=-10, max=10)
    std = torch.exp(0.5 * logvar)
    z = (mu + std * eps_z).unsqueeze(-1).unsqueeze(-1)
    recon = R.generator_forward(m.G, m.g_spec, z, True)
    real_labels = torch.full((B,), 0.9, dtype=dt)
    fake_labels = torch.full((B,), 0.1, dtype=dt)
    real_noisy = clean + 0.05 * eps_real
    recon_noisy = recon + 0.05 * eps_recon
    d_losses = []
    for _ in range(2):
        real_out = R.discriminator_forward(m.D, m.d_spec, real_noisy, True)
        fake_out = R.discriminator_forward(m.D, m.d_spec, recon_noisy.detach(), True)
        d_loss = R.bce_loss(real_out, real_labels) + R.bce_loss(fake_out, fake_labels)
        m.opt_D.zero_grad()
        d_loss.backward()
        m.opt_D.step()
        d_losses.append(float(d_loss.detach()))
    fake_out = R.discriminator_forward(m.D, m.d_spec, recon_noisy, True)
    weighted = rects is not None and hole_weight != 1.0
    hole = None
    if weighted:
        recon_loss, hole = weighted_mse(recon, clean, rects, hole_weight)
    else:
        recon_loss = R.mse_loss(recon, clean)
    kl_loss = R.kl_sum(mu, logvar) / B
    g_loss_adv = R.bce_loss(fake_out, real_labels)
    total = recon_loss + alpha_kl * min(1.0, epoch / 50) * kl_loss + alpha_adv * g_loss_adv
    m.opt_E.zero_grad()
    m.opt_G.zero_grad()
    total.backward()
    m.opt_E.step()
    m.opt_G.step()
    out = {"recon_loss": float(recon_loss.detach()), "kl_loss": float(kl_loss.detach()), "g_loss_adv": float(g_loss_adv.detach()),
           "d_loss_1": d_losses[0], "d_loss_2": d_losses[1], "total": float(total.detach())}
    if weighted:
        out["hole_mse"] = float(hole.detach())
    return out


def ref_vae_step(model, img, noisy, eps_z, epoch, rects=None, hole_weight=1.0):
    """siblings_ref.RefVAE.train_step (main_vae.py:103-127) with the Encoder fed `noisy` in place of clamp(img + sigma
    eps_img), and the region-weighted term as in ref_step."""
    m = model
    mu, logvar = R.encoder_forward(m.E, noisy, True)
    logvar = torch.clamp(logvar, min=-10, max=10)
    std = torch.exp(0.5 * logvar)
    z = (mu + std * eps_z).unsqueeze(-1).unsqueeze(-1)
    recon = R.generator_forward(m.G, m.g_spec, z, True)
    weighted = rects is not None and hole_weight != 1.0
    hole = None
    if weighted:
        recon_loss, hole = weighted_mse(recon, img, rects, hole_weight)
    else:
        recon_loss = R.mse_loss(recon, img)
    kl_loss = R.kl_sum(mu, logvar)
    total = recon_loss + kl_loss * min(epoch / 50, 1.0) * 1e-5
    m.opt.zero_grad()
    total.backward()
    m.opt.step()
    out = {"recon_loss": float(recon_loss.detach()), "kl_loss": float(kl_loss.detach()), "total": float(total.detach())}
    if weighted:
        out["hole_mse"] = float(hole.detach())
    return out


# ---- the evaluation pass ---------------------------------------------------------------------------------------------
def psnr01(mse):
    """PSNR of images in [-1, 1] on the [0, 1] scale: ((a + 1)/2 - (b + 1)/2)^2 = (a - b)^2 / 4; inf for 0."""
    return math.inf if mse == 0 else 10.0 * math.log10(4.0 / mse)


def ref_paired_regions(batches):
    """batches: [(recon, noisy, clean, rects)] on the host -> the keys paired_test_epoch(regions=True) adds."""
    acc = {"": [0.0, 0.0, 0, 0], "_noisy": [0.0, 0.0, 0, 0]}
    for recon, noisy, clean, rects in batches:
        for suffix, x in (("", recon), ("_noisy", noisy)):
            _, _, s_hole, s_valid, n_hole, n_valid = region_mse(x, clean, rects, 1.0)
            for k, v in enumerate((s_hole, s_valid, n_hole, n_valid)):
                acc[suffix][k] += v
    out = {}
    for suffix, (s_hole, s_valid, n_hole, n_valid) in acc.items():
        m_hole = s_hole / n_hole if n_hole else 0.0
        m_valid = s_valid / n_valid if n_valid else 0.0
        out.update({"mse_hole" + suffix: m_hole, "mse_valid" + suffix: m_valid, "psnr_hole" + suffix: psnr01(m_hole),
                    "psnr_valid" + suffix: psnr01(m_valid), "hole_fraction" + suffix: n_hole / (n_hole + n_valid)})
    return out
