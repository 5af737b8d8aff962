"""Test infrastructure for the prior stream (decoded prior samples as the third Discriminator input; Larsen et al. 2016,
algorithm 1), CPU only:

  prior_forward / head_backward_g / nhwc_grad_tanh   numpy restatements of the contracts of vg_prior_forward,
                                 vg_head_backward_g and vg_nhwc_grad_tanh_to_nhwc (include/vaegan_hip.h), in f64 (and, where
                                 the contract is exact, in the storage type);
  ref_step                       oracle/vaegan_ref.RefVAEGAN.train_step with the stream's six steps added, written with that
                                 module's own functions (the oracle is imported, not edited); the options it composes with
                                 (augmentation table, feature loss, degraded pairs) come from the restatements that already
                                 exist for them.
"""
import numpy as np
import torch

import vaegan_ref as R
from _diffaug_ref import torch_closed
from _featloss_ref import d_forward_tapped
from _pairloss_ref import weighted_mse

U = 2.0 ** -24          # unit roundoff of f32

LOSS_KEYS = ("recon_loss", "kl_loss", "g_loss_adv", "d_loss_1", "d_loss_2", "feat_loss", "g_loss_adv_prior")


# ---- the kernel contracts --------------------------------------------------------------------------------------------
def bf16_round(a):
    """f32 -> the nearest bf16 (ties to even), returned as f32."""
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def prior_forward(eps, ZP, bf16=False):
    """z [B, ZP] = eps [B, L] with zero pad columns, in the storage type's values (f32 exact, bf16 round-to-nearest-even)."""
    eps = np.asarray(eps, dtype=np.float32)
    B, L = eps.shape
    z = np.zeros((B, ZP), dtype=np.float32)
    z[:, :L] = bf16_round(eps) if bf16 else eps
    return z


def bce_terms(p, t):
    """nn.BCELoss per element in f64: -(t max(log p, -100) + (1 - t) max(log(1 - p), -100))."""
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return -(t * np.maximum(np.log(p), -100.0) + (1.0 - t) * np.maximum(np.log1p(-p), -100.0))


def head_backward_g(p, x, w, B, targets, gscale, C, HW):
    """-> (loss, dlogit [R], dx [R, K], dw [C, HW]) in f64 for R = len(targets) * B rows: loss = sum of the groups' BCE means,
    dlogit = gscale (p - t) / max(p (1 - p), 1e-12) / B * p (1 - p), dx = dlogit w^T, dw[c, hw] = sum_r dlogit[r] x[r, hw C + c]
    (x is NHWC-flattened, dw in the reference's [1][C][kh][kw] layout)."""
    p = np.asarray(p, dtype=np.float64)
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    t = np.repeat(np.asarray(targets, dtype=np.float64), B)
    loss = sum(bce_terms(p[g * B:(g + 1) * B], tg).mean() for g, tg in enumerate(targets))
    pq = p * (1.0 - p)
    dlogit = gscale * (p - t) / np.maximum(pq, 1e-12) / B * pq
    dx = dlogit[:, None] * w[None, :]
    dw = (dlogit[:, None] * x).sum(0).reshape(HW, C).T.copy()
    return loss, dlogit, dx, dw


def nhwc_grad_tanh(add, t, CP):
    """dx [B, H, W, CP] = add * (1 - t^2) in f64: add [B, H, W, CP] engine layout, t [B, C, H, W]; pad channels zero."""
    add, t = np.asarray(add, dtype=np.float64), np.asarray(t, dtype=np.float64)
    B, C, H, W = t.shape
    dx = np.zeros((B, H, W, CP))
    dx[..., :C] = add[..., :C] * (1.0 - np.transpose(t, (0, 2, 3, 1)) ** 2)
    return dx


def prior_inputs(B, S, seed, latent=100):
    """(eps_prior [B, latent], eps_xp [B, 3, S, S]) ~ N(0, 1): the stream's two draws, next to _inputs.make_inputs(B, S, seed)."""
    g = torch.Generator().manual_seed(seed + 1_000_003)
    return torch.randn(B, latent, generator=g), torch.randn(B, 3, S, S, generator=g)


# ---- the iteration ---------------------------------------------------------------------------------------------------
def ref_step(model, real, eps_z, eps_real, eps_recon, epoch, eps_prior=None, eps_xp=None, prior_stream=False, alpha_kl=0.1,
             alpha_adv=0.1, feat_layer=None, alpha_feat=0.0, alpha_pix=1.0, table=None, cut=(0, 0), noisy=None, rects=None,
             hole_weight=1.0, cut_prior_grad=False, d_iters=2):
    """RefVAEGAN.train_step (vaegan_code.py:65-135) with, for prior_stream=True:
        1  z_p = eps_prior, x_p = G(z_p) in a second train-mode call AFTER the reconstruction's, xp_noisy = x_p + 0.05 eps_xp;
        3  d_loss = BCE(D(real_noisy), real) + BCE(D(recon_noisy.detach()), fake) + BCE(D(xp_noisy.detach()), fake), three
           train-mode calls in that order;
        4  g_loss_adv_prior = BCE(D(xp_noisy), real), called after the call on recon_noisy; total += alpha_adv * it.
    Options as in the restatements they come from: table / cut (_diffaug_ref: T on everything the Discriminator reads, prior
    sample b by row b), feat_layer / alpha_feat / alpha_pix (_featloss_ref: on the reconstruction only), noisy / rects /
    hole_weight (_pairloss_ref).  cut_prior_grad: the new term is evaluated but contributes no gradient (x_p detached in it).
    prior_stream=False and no option: the oracle's own iteration, operation for operation."""
    m = model
    B = real.size(0)
    dt = getattr(m, "dtype", torch.float32)
    real, eps_z, eps_real, eps_recon = (t.to(dt) for t in (real, eps_z, eps_real, eps_recon))
    T = (lambda x: x) if table is None else (lambda x: torch_closed(x, table, *cut))
    mu, logvar = R.encoder_forward(m.E, real if noisy is None else noisy.to(dt), True)
    logvar = torch.clamp(logvar, min=-10, max=10)
    std = torch.exp(0.5 * logvar)
    z = (mu + std * eps_z).unsqueeze(-1).unsqueeze(-1)
    recon = R.generator_forward(m.G, m.g_spec, z, True)
    x_p = None
    if prior_stream:
        z_p = eps_prior.to(dt).unsqueeze(-1).unsqueeze(-1)
        x_p = R.generator_forward(m.G, m.g_spec, z_p, True)
    real_labels = torch.full((B,), 0.9, dtype=dt)
    fake_labels = torch.full((B,), 0.1, dtype=dt)
    real_noisy = T(real + 0.05 * eps_real)
    recon_noisy = T(recon + 0.05 * eps_recon)
    xp_noisy = T(x_p + 0.05 * eps_xp.to(dt)) if prior_stream else None
    d_losses = [0.0, 0.0]
    for it in range(d_iters):
        real_out = R.discriminator_forward(m.D, m.d_spec, real_noisy, True)
        fake_out = R.discriminator_forward(m.D, m.d_spec, recon_noisy.detach(), True)
        d_loss = R.bce_loss(real_out, real_labels) + R.bce_loss(fake_out, fake_labels)
        if prior_stream:
            prior_out = R.discriminator_forward(m.D, m.d_spec, xp_noisy.detach(), True)
            d_loss = d_loss + R.bce_loss(prior_out, fake_labels)
        m.opt_D.zero_grad()
        d_loss.backward()
        m.opt_D.step()
        d_losses[min(it, 1)] = float(d_loss.detach())
    feat_loss = None
    if alpha_feat != 0.0:
        with torch.no_grad():
            _, f_real = d_forward_tapped(m.D, m.d_spec, real_noisy, feat_layer, True)
        fake_out, f_fake = d_forward_tapped(m.D, m.d_spec, recon_noisy, feat_layer, True)
        feat_loss = R.mse_loss(f_fake, f_real)
    else:
        fake_out = R.discriminator_forward(m.D, m.d_spec, recon_noisy, True)
    g_loss_adv_prior = None
    if prior_stream:
        prior_out = R.discriminator_forward(m.D, m.d_spec, xp_noisy.detach() if cut_prior_grad else xp_noisy, True)
        g_loss_adv_prior = R.bce_loss(prior_out, real_labels)
    weighted = rects is not None and hole_weight != 1.0
    hole = None
    if weighted:
        recon_loss, hole = weighted_mse(recon, real, rects, hole_weight)
    else:
        recon_loss = R.mse_loss(recon, real)
    kl_loss = R.kl_sum(mu, logvar) / B
    g_loss_adv = R.bce_loss(fake_out, real_labels)
    if alpha_pix == 1.0:
        total = recon_loss + alpha_kl * min(1.0, epoch / 50) * kl_loss + alpha_adv * g_loss_adv
    else:
        total = alpha_pix * recon_loss + alpha_kl * min(1.0, epoch / 50) * kl_loss + alpha_adv * g_loss_adv
    if feat_loss is not None:
        total = total + alpha_feat * feat_loss
    if prior_stream:
        total = total + alpha_adv * g_loss_adv_prior
    m.opt_E.zero_grad()
    m.opt_G.zero_grad()
    total.backward()
    m.opt_E.step()
    m.opt_G.step()
    out = {"recon_loss": float(recon_loss.detach()), "kl_loss": float(kl_loss.detach()),
           "g_loss_adv": float(g_loss_adv.detach()), "d_loss_1": d_losses[0], "d_loss_2": d_losses[1],
           "feat_loss": 0.0 if feat_loss is None else float(feat_loss.detach()), "total": float(total.detach())}
    if prior_stream:
        out["g_loss_adv_prior"] = float(g_loss_adv_prior.detach())
    if weighted:
        out["hole_mse"] = float(hole.detach())
    return out


def snapshot(model):
    """Every tensor of the oracle's three networks and optimizers, and every gradient, cloned."""
    out = {}
    for n, st, opt in (("E", model.E, model.opt_E), ("G", model.G, model.opt_G), ("D", model.D, model.opt_D)):
        for k, v in st.items():
            out[f"{n}.{k}"] = v.detach().clone()
            if v.grad is not None:
                out[f"{n}.{k}.grad"] = v.grad.detach().clone()
        for i, (a, b) in enumerate(zip(opt.exp_avg, opt.exp_avg_sq)):
            out[f"opt_{n}.{i}.m"], out[f"opt_{n}.{i}.v"] = a.clone(), b.clone()
    return out
