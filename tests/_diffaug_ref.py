"""Test infrastructure for the differentiable augmentation (include/vaegan_hip.h, "Differentiable augmentation"), CPU only:

  params_from_u24            vg_diffaug_params restated from the 24-bit values w >> 8 of the eight Philox words per image;
  forward / backward         the kernels' contract restated in numpy, operation for operation, in np.float32 (bitwise the
                             kernel on inputs where every intermediate is exact, and in general) or np.float64 (the reference
                             the error bounds are counted against);
  to_bf16 / from_bf16        round-to-nearest-even bf16 storage on uint16;
  torch_sequential           brightness -> saturation -> contrast -> translation -> cutout, the way DiffAugment writes them,
                             in torch on NCHW tensors (differentiable);
  torch_closed               the closed form of the contract in torch (differentiable; the identity table is exact);
  ref_step / ref_dcgan_step / ref_wgan_step
                             the oracle's iterations with the transform applied to what the Discriminator sees; the parameter
                             table is an argument (like _featloss_ref.ref_step, whose feature block is kept).
"""
import numpy as np
import torch

import vaegan_ref as R
from _featloss_ref import d_forward_tapped

U = 2.0 ** -24          # unit roundoff of f32
UB = 2.0 ** -8          # ... of bf16's 8 significant bits
PART = 1024             # pixels per part of the whole-image sum
BIG = 2.0 ** 30
BRIGHTNESS, SATURATION, CONTRAST, TRANSLATION, CUTOUT = 1, 2, 4, 8, 16
IDENTITY_ROW = (0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0)


def shift_range(size):
    """floor(size / 8 + 0.5)"""
    return (size + 4) // 8


def cut_size(size):
    """floor(size / 2 + 0.5)"""
    return (size + 1) // 2


def cut_of(policy, H, W):
    return (cut_size(H), cut_size(W)) if policy & CUTOUT else (0, 0)


def identity_table(B):
    return np.tile(np.array(IDENTITY_ROW, dtype=np.float32), (B, 1))


# ---- test inputs ------------------------------------------------------------------------------------------------------
def random_table(rng, PB, H, W, cut=True):
    t = identity_table(PB)
    t[:, 0] = rng.uniform(-0.5, 0.5, PB)
    t[:, 1] = rng.uniform(0, 2, PB)
    t[:, 2] = rng.uniform(0.5, 1.5, PB)
    t[:, 3] = rng.integers(-shift_range(H), shift_range(H) + 1, PB)
    t[:, 4] = rng.integers(-shift_range(W), shift_range(W) + 1, PB)
    if cut:
        ch, cw = cut_size(H), cut_size(W)
        t[:, 5] = rng.integers(0, H + 1 - ch % 2, PB) - ch // 2
        t[:, 6] = rng.integers(0, W + 1 - cw % 2, PB) - cw // 2
    return t


def exact_case(N, H, W, C, PB, seed):
    """Inputs on which every intermediate of the contract is exact in f32 AND in bf16 storage of the result is not needed:
    x in multiples of 3 from +-3 .. +-9, s, k in {0.5, 1, 1.5, 2}, beta in {0, +-0.25}, H W a power of two."""
    rng = np.random.default_rng(seed)
    x = (rng.integers(1, 4, (N, H, W, C)) * 3 * rng.choice([-1, 1], (N, H, W, C))).astype(np.float32)
    t = identity_table(PB)
    t[:, 0] = rng.choice([0.0, 0.25, -0.25], PB)
    t[:, 1] = rng.choice([0.5, 1.0, 1.5, 2.0], PB)
    t[:, 2] = rng.choice([0.5, 1.0, 1.5, 2.0], PB)
    t[:, 3] = rng.integers(-2, 3, PB)
    t[:, 4] = rng.integers(-2, 3, PB)
    t[:, 5] = rng.integers(-1, H, PB)
    t[:, 6] = rng.integers(-1, W, PB)
    return x, t


# ---- the parameter generator -----------------------------------------------------------------------------------------
def _rint(u24, lo, hi):
    """lo + ((w >> 8) * (hi - lo) >> 24) in integer arithmetic"""
    return lo + ((u24.astype(np.int64) * (hi - lo)) >> 24)


def params_from_u24(u24, policy, H, W):
    """u24: integer array [B, 8], u24[b][i] = word(VG_DRAW_AUGMENT, 8 b + i) >> 8.  -> f32 [B, 8]."""
    u24 = np.asarray(u24, dtype=np.int64)
    B = u24.shape[0]
    u01 = (u24.astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
    out = identity_table(B)
    if policy & BRIGHTNESS:
        out[:, 0] = u01[:, 0] - np.float32(0.5)
    if policy & SATURATION:
        out[:, 1] = np.float32(2.0) * u01[:, 1]
    if policy & CONTRAST:
        out[:, 2] = u01[:, 2] + np.float32(0.5)
    if policy & TRANSLATION:
        out[:, 3] = _rint(u24[:, 3], -shift_range(H), shift_range(H) + 1).astype(np.float32)
        out[:, 4] = _rint(u24[:, 4], -shift_range(W), shift_range(W) + 1).astype(np.float32)
    if policy & CUTOUT:
        ch, cw = cut_size(H), cut_size(W)
        out[:, 5] = (_rint(u24[:, 5], 0, H + 1 - ch % 2) - ch // 2).astype(np.float32)
        out[:, 6] = (_rint(u24[:, 6], 0, W + 1 - cw % 2) - cw // 2).astype(np.float32)
    return out


# ---- bf16 storage ----------------------------------------------------------------------------------------------------
def to_bf16(a):
    """f32 array -> uint16 bf16 bits, round to nearest even (NaN stays NaN)."""
    bits = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    rounded = (bits + 0x7FFF + ((bits >> 16) & 1)) >> 16
    nan = np.isnan(a)
    return np.where(nan, 0x7FC0, rounded).astype(np.uint16)


def from_bf16(b):
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


# ---- the contract, operation for operation ---------------------------------------------------------------------------
def _int_slot(v):
    """An integer carried in f32: (value truncated toward zero, ok); NaN or |v| >= 2^30: (0, False)."""
    v = float(v)
    ok = abs(v) < BIG                   # False for NaN
    return (int(v) if ok else 0), ok


def source_index(row, H, W, cut_h, cut_w, bwd):
    """int array [H, W]: the source pixel hs * W + ws each destination pixel reads, -1 where it reads zeros."""
    ty, _ = _int_slot(row[3])
    tx, _ = _int_slot(row[4])
    cy, oky = _int_slot(row[5])
    cx, okx = _int_slot(row[6])
    cut = cut_h > 0 and cut_w > 0 and oky and okx
    hh, ww = np.mgrid[0:H, 0:W]
    hs, ws = (hh - ty, ww - tx) if bwd else (hh + ty, ww + tx)
    inside = (hs >= 0) & (hs < H) & (ws >= 0) & (ws < W)
    th, tw = (hs, ws) if bwd else (hh, ww)                      # where the cutout is tested
    masked = cut & (th >= cy) & (th < cy + cut_h) & (tw >= cx) & (tw < cx + cut_w)
    return np.where(inside & ~masked, hs * W + ws, -1)


def image_sum(sc, dt):
    """The whole-image sum of the per-pixel channel sums sc [H W], in the kernel's fixed order."""
    HW = sc.shape[0]
    parts = (HW + PART - 1) // PART
    a = np.zeros(parts * PART, dtype=dt)
    a[:HW] = sc
    a = a.reshape(parts, 4, 256)                                # pixel 1024 q + 256 j + t
    v = (a[:, 0] + a[:, 1]) + (a[:, 2] + a[:, 3])               # [parts, 256]
    v = v.reshape(parts, 4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lane ^ o]
    w = v[:, :, 0]
    part = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    S = dt(0)
    for q in range(parts):
        S = dt(S + part[q])
    return S


def _apply(x, params, cut_h, cut_w, dt, bwd, need_sum):
    x = np.asarray(x)
    N, H, W, C = x.shape
    params = np.asarray(params, dtype=np.float32)
    PB = params.shape[0]
    assert N % PB == 0
    HW = H * W
    out = np.zeros((N, HW, C), dtype=dt)
    for n in range(N):
        row = params[n % PB]
        beta, s, k = dt(row[0]), dt(row[1]), dt(row[2])
        src = source_index(row, H, W, cut_h, cut_w, bwd).reshape(HW)
        flat = x[n].reshape(HW, C).astype(dt)
        live = src >= 0
        v = np.where(live[:, None], flat[np.where(live, src, 0)], dt(0))

        def chan_sum(a):
            sc = np.zeros(HW, dtype=dt)
            for c in range(C):
                sc = sc + a[:, c]
            return sc
        sc = chan_sum(v)
        ks = dt(k * s)
        b = dt(k - ks)
        c = dt(dt(1) - k)
        S = dt(0)
        if need_sum:
            S = image_sum(sc if bwd else chan_sum(flat), dt)
        mean = dt(S / dt(C * HW))
        cm = dt(c * mean)
        e = cm if bwd else dt(cm + beta)
        m = sc / dt(C)
        o = ((ks * v) + (b * m)[:, None]) + e
        if not bwd:
            o = np.where(live[:, None], o, dt(0))
        out[n] = o
    return out.reshape(N, H, W, C)


def forward(x, params, cut_h, cut_w, dt=np.float32, need_sum=True):
    """x [N, H, W, C] (real channels only) -> T(x) in dt arithmetic, before the rounding of the store."""
    return _apply(x, params, cut_h, cut_w, dt, False, need_sum)


def backward(g, params, cut_h, cut_w, dt=np.float32, need_sum=True):
    return _apply(g, params, cut_h, cut_w, dt, True, need_sum)


def abs_budget(x, params, cut_h, cut_w, bwd):
    """A = |ks| |v| + (|k| + |ks|) mean_c |v| + |1 - k| mean |.| + |beta|: the magnitude every rounding of the contract is
    relative to (the terms of out before cancellation), in f64, per element."""
    x = np.asarray(x, dtype=np.float64)
    N, H, W, C = x.shape
    params = np.asarray(params, dtype=np.float32).astype(np.float64)
    out = np.zeros((N, H * W, C))
    for n in range(N):
        row = params[n % params.shape[0]]
        beta, s, k = row[0], row[1], row[2]
        src = source_index(row, H, W, cut_h, cut_w, bwd).reshape(-1)
        flat = np.abs(x[n].reshape(H * W, C))
        live = src >= 0
        v = np.where(live[:, None], flat[np.where(live, src, 0)], 0.0)
        tot = (v if bwd else flat).sum() / (C * H * W)
        out[n] = abs(k * s) * v + (abs(k) + abs(k * s)) * v.mean(axis=1, keepdims=True) + abs(1 - k) * tot \
            + (0.0 if bwd else abs(beta))
    return out.reshape(N, H, W, C)


def roundings(C, H, W):
    """The longest chain of f32 roundings between an input and an output of the contract: C - 1 channel additions, 2 + 6 + 3 for
    the thread's four pixels, the butterfly and the four waves, one per part, the quotient by C H W, c = 1 - k, c * mean,
    + beta, and the two additions of out_c (the chains through ks = k s and b = k - ks, m = sc / C are shorter)."""
    return (C - 1) + 11 + (H * W + PART - 1) // PART + 4 + 2


# ---- torch forms (NCHW, differentiable) ------------------------------------------------------------------------------
def _geometry(y, row, cut_h, cut_w):
    """Translation and cutout of one image col [C, H, W] by `row` (a sequence of 8 numbers)."""
    C, H, W = y.shape
    idx = torch.as_tensor(source_index(np.asarray([float(v) for v in row], dtype=np.float32), H, W, cut_h, cut_w, False))
    live = idx >= 0
    g = y.reshape(C, H * W)[:, idx.clamp_min(0).reshape(-1)].reshape(C, H, W)
    return torch.where(live.unsqueeze(0), g, torch.zeros((), dtype=y.dtype))


def torch_sequential(x, table, cut_h, cut_w):
    """x [N, C, H, W]; table [PB, 8]; image n uses row n % PB."""
    out = []
    for n in range(x.shape[0]):
        row = [float(v) for v in table[n % len(table)]]
        beta, s, k = row[0], row[1], row[2]
        y = x[n] + beta                                          # brightness
        m = y.mean(dim=0, keepdim=True)
        y = (y - m) * s + m                                      # saturation about the channel mean
        M = y.mean()
        y = (y - M) * k + M                                      # contrast about the image mean
        out.append(_geometry(y, row, cut_h, cut_w))
    return torch.stack(out)


def torch_closed(x, table, cut_h, cut_w):
    """The contract's closed form: k s x + (k - k s) m + (1 - k) M + beta with m, M the means of the SOURCE image."""
    out = []
    for n in range(x.shape[0]):
        row = [float(v) for v in table[n % len(table)]]
        beta, s, k = row[0], row[1], row[2]
        ks = k * s
        y = ks * x[n] + (k - ks) * x[n].mean(dim=0, keepdim=True) + (1.0 - k) * x[n].mean() + beta
        out.append(_geometry(y, row, cut_h, cut_w))
    return torch.stack(out)


# ---- the iterations --------------------------------------------------------------------------------------------------
def ref_step(model, real, eps_z, eps_real, eps_recon, epoch, table, cut=(0, 0), alpha_kl=0.1, alpha_adv=0.1, feat_layer=None,
             alpha_feat=0.0, alpha_pix=1.0, noisy=None):
    """RefVAEGAN.train_step (vaegan_code.py:65-135; the feature block of _featloss_ref.ref_step kept) with T(table) applied to
    both batches the Discriminator sees, image b and reconstruction b by row b.  table None: the oracle's iteration itself.
    noisy: the paired step (the Encoder reads it instead of real)."""
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
    real_labels = torch.full((B,), 0.9, dtype=dt)
    fake_labels = torch.full((B,), 0.1, dtype=dt)
    real_noisy = T(real + 0.05 * eps_real)
    recon_noisy = T(recon + 0.05 * eps_recon)
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


def ref_dcgan_step(o, real, noise, table, cut=(0, 0)):
    """oracle/siblings_ref.RefDCGAN.train_step with T(table) on every Discriminator input."""
    T = (lambda x: x) if table is None else (lambda x: torch_closed(x, table, *cut))
    B = real.size(0)
    ones, zeros = torch.ones(B, dtype=real.dtype), torch.zeros(B, dtype=real.dtype)
    o.opt_D.zero_grad()
    errD_real = R.bce_loss(o._d(T(real)), ones)
    errD_real.backward()
    fake = o._g(noise)
    errD_fake = R.bce_loss(o._d(T(fake.detach())), zeros)
    errD_fake.backward()
    o.opt_D.step()
    o.opt_G.zero_grad()
    errG = R.bce_loss(o._d(T(fake)), ones)
    errG.backward()
    o.opt_G.step()
    return {"errD_real": float(errD_real.detach()), "errD_fake": float(errD_fake.detach()), "errG": float(errG.detach())}


def ref_wgan_step(o, real, critic_noise, gen_noise, table, cut=(0, 0), clip_value=0.01):
    """oracle/siblings_ref.RefWGAN.train_step with T(table) on every critic input (one table for the whole step)."""
    T = (lambda x: x) if table is None else (lambda x: torch_closed(x, table, *cut))
    d_loss = None
    for z in critic_noise:
        o.opt_D.zero_grad()
        d_loss_real = -o._d(T(real)).mean()
        with torch.no_grad():
            fake = o._g(z)
        d_loss_fake = o._d(T(fake)).mean()
        d_loss = d_loss_real + d_loss_fake
        d_loss.backward()
        o.opt_D.step()
        with torch.no_grad():
            for p in o.opt_D.params:
                p.clamp_(-clip_value, clip_value)
    o.opt_G.zero_grad()
    g_loss = -o._d(T(o._g(gen_noise))).mean()
    g_loss.backward()
    o.opt_G.step()
    return {"d_loss": float(d_loss.detach()), "g_loss": float(g_loss.detach())}
