"""Test infrastructure for the Discriminator-feature reconstruction loss (Larsen et al. 2016, eq. 2), CPU only:

  feat_mse / feat_mse_grad_add   f64 restatement of the contract of vg_feat_mse_forward_backward (include/vaegan_hip.h);
  stage_prefix_len / d_forward_tapped   the map from an engine stage of the Discriminator to the oracle's Sequential spec;
  ref_step                       oracle/vaegan_ref.RefVAEGAN.train_step with the feature-loss block added, written with
                                 that module's own functions (the oracle is imported, not edited).
"""
import torch

import vaegan_ref as R

U = 2.0 ** -24          # unit roundoff of f32
UB = 2.0 ** -8          # ... of bf16's 8 significant bits


# ---- the kernel contract in f64 --------------------------------------------------------------------------------------
def feat_mse(a, b):
    """(1/n) sum (a - b)^2"""
    a, b = a.double().flatten(), b.double().flatten()
    return ((a - b) ** 2).sum() / a.numel()


def feat_mse_grad_add(a, b, d_in, gscale):
    """-> (g, d_in + g) with g = gscale 2 (a - b) / n, the gradient of gscale * feat_mse w.r.t. a (b is a constant)."""
    a, b = a.double().flatten(), b.double().flatten()
    g = gscale * 2.0 * (a - b) / a.numel()
    return g, (g if d_in is None else d_in.double().flatten() + g)


# ---- engine stage -> oracle spec -------------------------------------------------------------------------------------
def feature_stages(spec):
    """Engine stages of the Discriminator `spec` that have a BatchNorm: stage 0 is (conv, lrelu), stage i >= 1 is
    (conv, bn, lrelu) at spec indices 3i - 1 .. 3i + 1, the head (conv, sigmoid) comes last."""
    n_stages = (len(spec) - 2 - 2) // 3 + 1          # without the head
    return list(range(1, n_stages))


def stage_prefix_len(spec, l):
    """Number of leading spec entries whose output is the ACTIVATED output of engine stage l (>= 1): up to and including
    the LeakyReLU at spec index 3 l + 1."""
    if l not in feature_stages(spec):
        raise ValueError(f"stage {l} has no BatchNorm")
    k = 3 * l + 2
    assert spec[k - 3][0] == "conv" and spec[k - 2][0] == "bn" and spec[k - 1][0] == "lrelu"
    return k


def _shifted(st, k):
    """The same tensors under the keys a Sequential that starts at entry k would use (sequential_forward numbers the
    entries of the spec it is given from 0); in-place BatchNorm buffer updates reach the original state."""
    out = {}
    for key, v in st.items():
        _, idx, name = key.split(".", 2)
        if int(idx) >= k:
            out[f"main.{int(idx) - k}.{name}"] = v
    return out


def d_forward_tapped(st, spec, x, l, train=True):
    """One call of the Discriminator, tapped at stage l: -> (probabilities [B], D_l(x)).  The whole stack runs."""
    k = stage_prefix_len(spec, l)
    f = R.sequential_forward(st, spec[:k], x, train)
    p = R.sequential_forward(_shifted(st, k), spec[k:], f, train).view(-1)
    return p, f


# ---- the iteration ---------------------------------------------------------------------------------------------------
def ref_step(model, real, eps_z, eps_real, eps_recon, epoch, alpha_kl=0.1, alpha_adv=0.1, feat_layer=None,
             alpha_feat=0.0, alpha_pix=1.0):
    """RefVAEGAN.train_step (vaegan_code.py:65-135) with, for alpha_feat != 0, the learned-similarity term:
        f_real = D_l(real_noisy)   under no_grad, one more train-mode call of D after the two D updates
        fake_out, f_fake = D(recon_noisy) tapped at l           (the existing call :110)
        total = alpha_pix recon + alpha_kl min(1, epoch/50) kl + alpha_adv adv + alpha_feat mse(f_fake, f_real)."""
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
    feat_loss = None
    if alpha_feat != 0.0:
        with torch.no_grad():
            _, f_real = d_forward_tapped(m.D, m.d_spec, real_noisy, feat_layer, True)
        fake_out, f_fake = d_forward_tapped(m.D, m.d_spec, recon_noisy, feat_layer, True)
        feat_loss = R.mse_loss(f_fake, f_real)
    else:
        fake_out = R.discriminator_forward(m.D, m.d_spec, recon_noisy, True)
    recon_loss = R.mse_loss(recon, real)
    kl_loss = R.kl_sum(mu, logvar) / B
    g_loss_adv = R.bce_loss(fake_out, real_labels)
    total = alpha_pix * recon_loss + alpha_kl * min(1.0, epoch / 50) * kl_loss + alpha_adv * g_loss_adv
    if feat_loss is not None:
        total = total + alpha_feat * feat_loss
    m.opt_E.zero_grad()
    m.opt_G.zero_grad()
    total.backward()
    m.opt_E.step()
    m.opt_G.step()
    return {"recon_loss": float(recon_loss.detach()), "kl_loss": float(kl_loss.detach()),
            "g_loss_adv": float(g_loss_adv.detach()), "d_loss_1": d_losses[0], "d_loss_2": d_losses[1],
            "feat_loss": 0.0 if feat_loss is None else float(feat_loss.detach()), "total": float(total.detach())}
