"""Test infrastructure for gradient-norm clipping (include/vaegan_hip.h "Gradient-norm clipping"), CPU only:

  norm_coef              the contract of vg_grad_norm_clip restated in numpy f64 / f32: (norm, coef) as the two f32 it writes;
  clip_scale             s = grad_scale * coef, the one rounded f32 product vg_adam_apply_clip forms;
  clipped_adam_step      torch.optim.Adam (single-tensor f32 form, CPU) fed g * s;
  int_grads / float_grads   inputs: integer-valued gradients in {-3 .. 3} (S is then exact in f64 whatever the order of the
                         sum, so a kernel must agree BIT FOR BIT) and random floats over several decades;
  check_conditions       the exactness premise of the integer inputs, S < 2^53;
  ref_step / ref_vae_step   the oracle's iterations (oracle/vaegan_ref.RefVAEGAN, oracle/siblings_ref.RefVAE; imported, not
                         edited) with torch.nn.utils.clip_grad_norm_ inserted before each optimizer step.
"""
import math

import numpy as np
import torch

import vaegan_ref as R

F32 = np.float32
NETS = ("E", "G", "D")


# ---- the kernel contract ---------------------------------------------------------------------------------------------
def sum_squares(g: np.ndarray) -> float:
    """S = sum_j (double)g[j]^2: every product exact in f64 (24-bit significands), the sum in f64.  An f64 array (the f64
    oracle's gradients) is taken as it is; anything else is an f32 buffer."""
    g = np.asarray(g)
    d = (g if g.dtype == np.float64 else g.astype(F32).astype(np.float64)).ravel()
    with np.errstate(over="ignore", invalid="ignore"):
        return float(np.sum(d * d))


def norm_coef_f64(g, grad_scale, max_norm):
    """-> (norm, c) in f64, before the narrowing: norm = |f32(grad_scale)| sqrt(S), c = clamp(max_norm / (norm + 1e-6), max=1)
    with a NaN kept (torch.clamp keeps it; fmin would not)."""
    with np.errstate(all="ignore"):                      # numpy's f64 scalars follow IEEE through inf and NaN
        S = np.float64(sum_squares(g))
        norm = np.abs(np.float64(F32(grad_scale))) * np.sqrt(S)
        c = np.float64(max_norm) / (norm + np.float64(1e-6))
    return float(norm), float(c if c < 1.0 else (c if c != c else 1.0))


def norm_coef(g, grad_scale, max_norm):
    """-> (out[0], out[1]) of vg_grad_norm_clip as np.float32, each narrowed once from the f64 value."""
    norm, c = norm_coef_f64(g, grad_scale, max_norm)
    with np.errstate(over="ignore"):
        return np.float64(norm).astype(F32), np.float64(c).astype(F32)


def clip_scale(grad_scale, coef) -> np.float32:
    """s of vg_adam_apply_clip: one rounded f32 product; coef None (a NULL entry): grad_scale as it is."""
    return F32(grad_scale) if coef is None else F32(F32(grad_scale) * F32(coef))


def bits(x) -> np.ndarray:
    return np.asarray(x, dtype=F32).reshape(-1).view(np.int32)


def same_bits(a, b) -> bool:
    """Equal f32 bit patterns, except that any NaN equals any NaN (the payload of a computed NaN is not in the contract)."""
    a, b = np.asarray(a, dtype=F32).reshape(-1), np.asarray(b, dtype=F32).reshape(-1)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and bool(np.array_equal(na, nb)) and bool(np.array_equal(a[~na].view(np.int32), b[~nb].view(np.int32)))


def ulp_distance(a, b) -> int:
    """Distance of two finite f32 of one sign in units in the last place."""
    return abs(int(F32(a).view(np.int32)) - int(F32(b).view(np.int32)))


# ---- inputs ----------------------------------------------------------------------------------------------------------
def int_grads(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(-3, 4, size=n).astype(F32)


def float_grads(n: int, seed: int) -> np.ndarray:
    """randn times 10^u, u uniform in [-4, 2): magnitudes over six decades, both signs."""
    r = np.random.default_rng(seed)
    return (r.standard_normal(n) * 10.0 ** r.uniform(-4.0, 2.0, size=n)).astype(F32)


def pow2_norm_grads(n: int, seed: int):
    """-> (g, norm): integer-valued gradients in {-3 .. 3} times a power of two whose L2 norm is EXACTLY a power of two >= 64.
    Every partial sum of squares is an integer below 2^24, so torch's f32 reduction and the kernel's f64 one both give that
    norm exactly, and for max_norm = norm / 2^j both coefficients are 2^-j exactly: in f32, norm + 1e-6 == norm (1e-6 is
    below half an ulp from 32 on); in f64, (norm / 2^j) / (norm + 1e-6) = 2^-j (1 - 1e-6 / norm) lies within 1.6e-8 relative
    of 2^-j, inside the half-spacing below a power of two (2^-25 relative = 3e-8), and narrows to it.  The two sides of a
    comparison with torch then hand Adam bit-identical gradients.
    Most elements are random; the first few are set so that the squares add up to 4^k (as many 3s as fit, then at most
    four smaller values, then zeros), and then shuffled in with random signs."""
    r = np.random.default_rng(seed)
    k = max(1, int(round(math.log(4.0 * n, 4.0))))
    T = 4 ** k
    m = min(n, 64 + int(8 * math.sqrt(n)))
    rest = r.integers(-3, 4, size=n - m).astype(np.int64)
    D = T - int(np.sum(rest * rest))
    assert 0 <= D <= 9 * m, (n, T, D, m)
    adj = []
    for _ in range(m):
        a = min(3, int(math.isqrt(D)))
        adj.append(a)
        D -= a * a
    assert D == 0, (n, T, D)
    v = np.concatenate([np.array(adj, dtype=np.int64) * r.choice([-1, 1], size=m), rest])
    r.shuffle(v)
    e = max(0, 6 - k)
    g = (v * 2 ** e).astype(F32)
    norm = float(2 ** (k + e))
    assert sum_squares(g) == norm * norm < 2.0 ** 24 and norm >= 64.0
    return g, norm


def check_conditions(g: np.ndarray) -> None:
    """The premise under which S does not depend on the order of the sum: integer-valued elements and S < 2^53 (every
    partial sum is then an integer below 2^53, exact in f64)."""
    assert np.array_equal(g, np.round(g)) and np.isfinite(g).all()
    assert sum_squares(g) < 2.0 ** 53


def max_norms_around(g, grad_scale):
    """Max norms above, below and (as nearly as f64 has it) equal to the norm of g: -> [2 norm, norm / 2, norm]."""
    norm, _ = norm_coef_f64(g, grad_scale, math.inf)
    return [2.0 * norm + 1.0, 0.5 * norm, norm]


# ---- the clipped Adam step -------------------------------------------------------------------------------------------
def clipped_adam_step(p0, grads, lr, betas, eps, grad_scale=1.0, coefs=None):
    """torch.optim.Adam (foreach=False, f32, CPU) over the gradients g_k * s_k, s_k = clip_scale(grad_scale, coefs[k]) -- what
    vg_adam_apply_clip is held to.  p0 / grads: f32 torch tensors.  -> (p, exp_avg, exp_avg_sq)."""
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps, foreach=False)
    for k, g in enumerate(grads):
        s = clip_scale(grad_scale, None if coefs is None else coefs[k])
        p.grad = g.clone() * torch.tensor(s)
        opt.step()
    st = opt.state[p]
    return p.detach(), st["exp_avg"], st["exp_avg_sq"]


# ---- the oracle's iterations with torch's clipping -------------------------------------------------------------------
def _max_for(max_norm, name):
    if isinstance(max_norm, dict):
        return max_norm.get(name)
    return max_norm


def _clip(opt, max_norm, seen, name):
    """torch's clip_grad_norm_ over the optimizer's parameters; records the flattened gradient it saw and returns the norm."""
    flat = torch.cat([q.grad.detach().reshape(-1) for q in opt.params if q.grad is not None]).clone()
    seen[name] = flat
    if max_norm is None:
        return None
    return float(torch.nn.utils.clip_grad_norm_(opt.params, max_norm, norm_type=2, error_if_nonfinite=False))


def ref_step(model, real, eps_z, eps_real, eps_recon, epoch, max_norm=None, d_iters=2, alpha_kl=0.1, alpha_adv=0.1):
    """RefVAEGAN.train_step (vaegan_code.py:65-135) with torch.nn.utils.clip_grad_norm_(params, max_norm) directly before each
    optimizer step, per network.  max_norm: None (no call), a number, or a dict over "E", "G", "D".
    -> losses as RefVAEGAN.train_step returns them, plus grad_norm_E / _G / _D (D: the last update's) where clipped, plus
    "seen": the flattened gradient each network's (last) clip call was handed, before it was scaled."""
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
    d_losses, seen, norms = [], {}, {}
    for _ in range(d_iters):
        real_out = R.discriminator_forward(m.D, m.d_spec, real_noisy, True)
        fake_out = R.discriminator_forward(m.D, m.d_spec, recon_noisy.detach(), True)
        d_loss = R.bce_loss(real_out, real_labels) + R.bce_loss(fake_out, fake_labels)
        m.opt_D.zero_grad()
        d_loss.backward()
        norms["D"] = _clip(m.opt_D, _max_for(max_norm, "D"), seen, "D")
        m.opt_D.step()
        d_losses.append(float(d_loss.detach()))
    fake_out = R.discriminator_forward(m.D, m.d_spec, recon_noisy, True)
    recon_loss = R.mse_loss(recon, real)
    kl_loss = R.kl_sum(mu, logvar) / B
    g_loss_adv = R.bce_loss(fake_out, real_labels)
    total = recon_loss + alpha_kl * min(1.0, epoch / 50) * kl_loss + alpha_adv * g_loss_adv
    m.opt_E.zero_grad()
    m.opt_G.zero_grad()
    total.backward()
    norms["E"] = _clip(m.opt_E, _max_for(max_norm, "E"), seen, "E")
    norms["G"] = _clip(m.opt_G, _max_for(max_norm, "G"), seen, "G")
    m.opt_E.step()
    m.opt_G.step()
    out = {"recon_loss": float(recon_loss.detach()), "kl_loss": float(kl_loss.detach()),
           "g_loss_adv": float(g_loss_adv.detach()), "d_loss_1": d_losses[0],
           "d_loss_2": d_losses[1] if d_iters > 1 else 0.0, "total": float(total.detach()), "seen": seen}
    out.update({f"grad_norm_{k}": v for k, v in norms.items() if v is not None})
    return out


def ref_vae_step(model, img, eps_img, eps_z, epoch, max_norm=None, noise_max_std=0.5):
    """siblings_ref.RefVAE.train_step (main_vae.py:103-127) with torch's clip_grad_norm_ before the one optimizer's step."""
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
    m.opt.zero_grad()
    total.backward()
    seen = {}
    norm = _clip(m.opt, max_norm, seen, "EG")
    m.opt.step()
    out = {"recon_loss": float(recon_loss.detach()), "kl_loss": float(kl_loss.detach()), "total": float(total.detach()),
           "seen": seen}
    if norm is not None:
        out["grad_norm_EG"] = norm
    return out

