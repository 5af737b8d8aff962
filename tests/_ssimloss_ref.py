"""Test infrastructure for the SSIM reconstruction loss (vg_ssim_loss_forward_backward, csrc/ssimloss.hip), CPU only:

  loss_and_grad          1 - mean SSIM and its gradient w.r.t. the first image, from tests/_pointwise_ref.ssim_map (the
                         explicit 11 x 11 window, tap by tap) through torch autograd; dtype=torch.float32 evaluates the
                         same graph in f32 (the yardstick of the f32 cancellation in E[x^2] - E[x]^2);
  closed_form            the contract of include/vaegan_hip.h written out: the three derivative maps and their transposed,
                         full correlation with the window, tap by tap, in f64, no autograd;
  grad_add               d + gscale * gradient: what the entry point leaves in d;
  activation_margin      how close the oracle's forward comes to a ReLU / LeakyReLU kink on a given input (see there);
  ref_step, ref_vae_step oracle/vaegan_ref.RefVAEGAN.train_step and oracle/siblings_ref.RefVAE.train_step with the one added
                         term, written with those modules' own functions (the oracles are imported, not edited).
"""
from unittest import mock

import torch

import _pointwise_ref as P
import vaegan_ref as R

U = P.U
C1, C2 = 0.01 ** 2, 0.03 ** 2


def ssim_loss(a, b, dtype=torch.float64):
    """1 - mean over the interior pixels of the SSIM map; a differentiable torch scalar of `dtype`."""
    return 1.0 - P.ssim_map(a, b, dtype).mean()


def loss_and_grad(a, b, dtype=torch.float64):
    """-> (loss, d loss / d a) as f64 tensors, evaluated in `dtype` by torch autograd through ssim_map.  b is a constant."""
    x = a.detach().to(dtype).clone().requires_grad_(True)
    loss = ssim_loss(x, b.detach().to(dtype), dtype)
    (g,) = torch.autograd.grad(loss, x)
    return loss.detach().double(), g.double()


def closed_form(a, b):
    """The contract, tap by tap, in f64 -> (loss, d loss / d a):
        Du = -A1 A2 / (B1 B2^2), Dc = 2 A1 / (B1 B2), Dm = 2 mu_v A2 / (B1 B2) - 2 mu_u A1 A2 / (B1^2 B2) - 2 mu_u Du - mu_v Dc
        d mean S / d a[q] = (1 / 2n) [ (w * Dm)(q) + 2 u(q) (w * Du)(q) + v(q) (w * Dc)(q) ]
    with * the transposed, full correlation with w = g (x) g (an interior pixel p reaches q = p + (dy, dx) - 5)."""
    u = (a.double() + 1) * 0.5
    v = (b.double() + 1) * 0.5
    g = P.gauss11()
    H, W = u.shape[-2:]
    IH, IW = H - 10, W - 10
    z = torch.zeros(u.shape[:2] + (IH, IW), dtype=torch.float64)
    mu, mv, suu, svv, suv = z.clone(), z.clone(), z.clone(), z.clone(), z.clone()
    for dy in range(11):
        for dx in range(11):
            w = g[dy] * g[dx]
            pu, pv = u[..., dy:dy + IH, dx:dx + IW], v[..., dy:dy + IH, dx:dx + IW]
            mu += w * pu
            mv += w * pv
            suu += w * pu * pu
            svv += w * pv * pv
            suv += w * pu * pv
    suu, svv, suv = suu - mu * mu, svv - mv * mv, suv - mu * mv
    A1, A2 = 2 * mu * mv + C1, 2 * suv + C2
    B1, B2 = mu * mu + mv * mv + C1, suu + svv + C2
    S = A1 * A2 / (B1 * B2)
    Du = -A1 * A2 / (B1 * B2 * B2)
    Dc = 2 * A1 / (B1 * B2)
    Dm = 2 * mv * A2 / (B1 * B2) - 2 * mu * A1 * A2 / (B1 * B1 * B2) - 2 * mu * Du - mv * Dc
    wm, wu, wc = torch.zeros_like(u), torch.zeros_like(u), torch.zeros_like(u)
    for dy in range(11):
        for dx in range(11):
            w = g[dy] * g[dx]
            wm[..., dy:dy + IH, dx:dx + IW] += w * Dm
            wu[..., dy:dy + IH, dx:dx + IW] += w * Du
            wc[..., dy:dy + IH, dx:dx + IW] += w * Dc
    n = S.numel()
    return 1.0 - S.sum() / n, -(wm + 2 * u * wu + v * wc) / (2 * n)


def grad_add(g, d_in, gscale):
    """What the entry point leaves in d: d_in + f32(gscale) * g (g = d loss / d a in f64)."""
    g = P.f32(gscale) * g
    return g if d_in is None else d_in.double() + g


# ---- conditioning of a gradient comparison ---------------------------------------------------------------------------
ISO_SEED = 7074         # tests/_inputs.make_inputs(4, 64, ISO_SEED): the input of the isolated gradient-path test


def activation_margin(model, real, eps_z):
    """Encoder -> reparameterisation -> Generator forward of `model` (a RefVAEGAN, train mode, its state left untouched) with
    every input of a ReLU / LeakyReLU recorded -> (smallest |pre-activation|, list of the recorded tensors).
    A gradient is a discontinuous function of the input wherever a pre-activation crosses zero: an implementation whose
    rounding puts one element on the other side of the kink gets that element's mask wrong, and the BatchNorm bias
    gradient of its channel -- a sum of ~1000 terms of either sign -- moves by about one term, ~1e-2 relative, which then
    spreads to every layer below.  fp32 forwards differ from the fp64 one by a few 1e-7 near zero (up to 6e-6 on the
    largest values), and the 2.2 million pre-activations of an S = 64, B = 4 forward come within 3e-7 of zero on most
    inputs: the CPU fp32 oracle itself flips 1 - 3 of them on about half of the seeds 7064 .. 7103 (seed 7064: 2 flips,
    margin 2.5e-7), and its gradients are then 4e-3 off the fp64 ones on EVERY tensor -- such an input measures luck, not
    an implementation.  The isolated gradient-path test therefore takes the first seed from 7064 on whose fp64 forward
    keeps every pre-activation at least 2e-6 from zero (7074: 2.26e-6; tests/test_ssimloss_cpu.py asserts it)."""
    rec = []
    relu, lrelu = R.F.relu, R.F.leaky_relu

    def spy_relu(x, *a, **k):
        rec.append(x.detach())
        return relu(x, *a, **k)

    def spy_lrelu(x, *a, **k):
        rec.append(x.detach())
        return lrelu(x, *a, **k)

    dt = getattr(model, "dtype", torch.float32)
    E, G = ({k: v.detach().clone() for k, v in st.items()} for st in (model.E, model.G))
    with mock.patch.object(R.F, "relu", spy_relu), mock.patch.object(R.F, "leaky_relu", spy_lrelu), torch.no_grad():
        mu, logvar = R.encoder_forward(E, real.to(dt), True)
        logvar = torch.clamp(logvar, min=-10, max=10)
        z = (mu + torch.exp(0.5 * logvar) * eps_z.to(dt)).unsqueeze(-1).unsqueeze(-1)
        R.generator_forward(G, model.g_spec, z, True)
    return min(float(x.abs().min()) for x in rec), rec


# ---- the iterations ------------------------------------------------------------------------------------------------
def ref_step(model, real, eps_z, eps_real, eps_recon, epoch, alpha_kl=0.1, alpha_adv=0.1, alpha_pix=1.0, alpha_ssim=0.0):
    """RefVAEGAN.train_step (vaegan_code.py:65-135) with, for alpha_ssim != 0,
        total = alpha_pix recon + alpha_kl min(1, epoch/50) kl + alpha_adv adv + alpha_ssim (1 - SSIM(recon, real))."""
    m = model
    B = real.size(0)
    dt = getattr(m, "dtype", torch.float32)
    real, eps_z, eps_real, eps_recon = (t.to(dt) for t in (real, eps_z, eps_real, eps_recon))
    mu, logvar = R.encoder_forward(m.E, real, True)
    logvar = torch.clamp(logvar, min=-10, max=10)
    std = torch.exp(0.5 * logvar)
    z = (mu + std * eps_z).unsqueeze(-1).unsqueeze(-1)
    recon = R.generator_forward(m.G, m.g_spec, z, True)
    real_labels = torch.full((B,), 0.9, dtype=dt)
    fake_labels = torch.full((B,), 0.1, dtype=dt)
    real_noisy = real + 0.05 * eps_real
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
    recon_loss = R.mse_loss(recon, real)
    kl_loss = R.kl_sum(mu, logvar) / B
    g_loss_adv = R.bce_loss(fake_out, real_labels)
    total = alpha_pix * recon_loss + alpha_kl * min(1.0, epoch / 50) * kl_loss + alpha_adv * g_loss_adv
    sl = None
    if alpha_ssim != 0.0:
        sl = ssim_loss(recon, real, dt)
        total = total + alpha_ssim * sl
    m.opt_E.zero_grad()
    m.opt_G.zero_grad()
    total.backward()
    m.opt_E.step()
    m.opt_G.step()
    return {"recon_loss": float(recon_loss.detach()), "kl_loss": float(kl_loss.detach()),
            "g_loss_adv": float(g_loss_adv.detach()), "d_loss_1": d_losses[0], "d_loss_2": d_losses[1],
            "ssim_loss": 0.0 if sl is None else float(sl.detach()), "total": float(total.detach())}


def ref_vae_step(model, img, eps_img, eps_z, epoch, noise_max_std=0.5, alpha_ssim=0.0):
    """siblings_ref.RefVAE.train_step (main_vae.py:103-127) with, for alpha_ssim != 0,
        total = recon + kl min(epoch/50, 1) 1e-5 + alpha_ssim (1 - SSIM(recon, img))."""
    m = model
    noisy = torch.clamp(img + eps_img * noise_max_std, -1.0, 1.0)
    mu, logvar = R.encoder_forward(m.E, noisy, True)
    logvar = torch.clamp(logvar, min=-10, max=10)
    std = torch.exp(0.5 * logvar)
    z = (mu + std * eps_z).unsqueeze(-1).unsqueeze(-1)
    recon = R.generator_forward(m.G, m.g_spec, z, True)
    recon_loss = R.mse_loss(recon, img)
    kl_loss = R.kl_sum(mu, logvar)
    total = recon_loss + kl_loss * min(epoch / 50, 1.0) * 1e-5
    sl = None
    if alpha_ssim != 0.0:
        sl = ssim_loss(recon, img, recon.dtype)
        total = total + alpha_ssim * sl
    m.opt.zero_grad()
    total.backward()
    m.opt.step()
    return {"recon_loss": float(recon_loss.detach()), "kl_loss": float(kl_loss.detach()),
            "ssim_loss": 0.0 if sl is None else float(sl.detach()), "total": float(total.detach())}
