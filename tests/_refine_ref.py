"""Test infrastructure for test-time latent refinement (denoise.LatentRefiner, csrc/refine.hip), CPU only:

  bn_act_backward_eval   the contract of vg_bn_act_backward_eval with its own roundings (f32 products, one rounding to storage);
  masked_mse_rows        f64 restatement of vg_masked_mse_rows (the hole rule is _pairloss_ref.region_mask, the rule of
                         vg_region_mse_forward_backward);
  LatentAdam             vg_latent_adam: f64 arithmetic from f32 state, each stored value rounded once, the wave's summation order;
  refine_loop            the whole loop in f64 with torch autograd over reference-shaped eval-mode networks (oracle/vaegan_ref);
  make_case              networks, targets G(z*) with a painted rectangle and a perturbed start, as the GPU tests use them.
"""
import math

import numpy as np
import torch

import vaegan_ref as R
from _pairloss_ref import region_mask

ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2
REAL_LABEL = 0.9
F32 = np.float32


def bf16_round(x):
    """f32 ndarray -> the nearest bf16 (ties to even), as f32."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=F32)).bfloat16().float().numpy()


# ---- (a) --------------------------------------------------------------------------------------------------------------
def bn_act_backward_eval(x, dy, scale, shift, act, slope, bf16=False):
    """x, dy: f32 ndarrays [rows, C] holding storage-type values; scale, shift f32 [C].  z = fmaf(scale, x, shift): the product
    of two f32 is exact in f64, so the f64 sum rounded to f32 is the fused result (up to a double rounding that cannot move a
    sign); dz = dy where z > 0, else 0 (ReLU) / dy * slope in f32 (LeakyReLU); dx = dz * scale in f32, rounded to storage."""
    x, dy, scale, shift = (np.asarray(t, dtype=F32) for t in (x, dy, scale, shift))
    z = (x.astype(np.float64) * scale.astype(np.float64) + shift.astype(np.float64)).astype(F32)
    with np.errstate(invalid="ignore"):
        pos = z > 0
    if act == ACT_RELU:
        dz = np.where(pos, dy, F32(0))
    elif act == ACT_LRELU:
        dz = np.where(pos, dy, dy * F32(slope))
    else:
        dz = dy
    out = (dz * scale).astype(F32)
    return bf16_round(out) if bf16 else out


EXACT_SLOPE = 0.25


def exact_case(seed, rows, C):
    """Inputs on which every f32 / bf16 operation of (a) is exact, so the reference is unique and a comparison bitwise:
    x nonzero integers in [-6, 6], dy nonzero multiples of 1/2 in [-6, 6], scale[c] = +-2^k (k in -2 .. 2, neighbours differ),
    shift[c] = -scale[c] a[c] with a[c] a nonzero integer in [-3, 3]: z = scale (x - a) is an integer multiple of 1/4, zero
    exactly where x == a -- forced in row 0, channels 0 .. 3, and frequent elsewhere.  Use with slope = EXACT_SLOPE."""
    rng = np.random.default_rng(seed)
    x = (rng.integers(1, 7, (rows, C)) * rng.choice([-1, 1], (rows, C))).astype(F32)
    dy = (rng.integers(1, 13, (rows, C)) * rng.choice([-1, 1], (rows, C)) * 0.5).astype(F32)
    c = np.arange(C)
    scale = (2.0 ** ((c * 3) % 5 - 2) * np.where(c % 3 == 2, -1.0, 1.0)).astype(F32)
    a = (c % 3 + 1) * np.where(c % 2 == 0, 1, -1)
    shift = (-scale * a).astype(F32)
    x[0, :4] = a[:4]
    return x, dy, scale, shift


# ---- (b) --------------------------------------------------------------------------------------------------------------
def masked_mse_rows(a, b, rects, gscale=1.0):
    """-> (loss_rows f64 [B], d_a f64 [B,C,H,W], n_valid int64 [B]): loss_rows[i] = S_valid_i / n_valid_i (0 without a valid
    element), d_a = 2 gscale (a - b) / n_valid_i outside the hole and 0 inside."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    B = a.shape[0]
    valid = ~region_mask(rects, *a.shape)
    d = a - b
    n_valid = valid.reshape(B, -1).sum(1)
    s = (d * d * valid).reshape(B, -1).sum(1)
    safe = n_valid.clamp(min=1).double()
    loss = torch.where(n_valid > 0, s / safe, torch.zeros_like(s))
    grad = 2.0 * float(F32(gscale)) * d * valid / safe.view(B, 1, 1, 1)
    return loss, grad, n_valid


def masked_mean_torch(recon, target, rects):
    """The per-image masked mean as a differentiable torch expression: -> [B]."""
    B = recon.shape[0]
    valid = (~region_mask(rects, *recon.shape)).to(recon.dtype)
    n_valid = valid.reshape(B, -1).sum(1)
    s = (((recon - target) ** 2) * valid).reshape(B, -1).sum(1)
    return torch.where(n_valid > 0, s / n_valid.clamp(min=1), torch.zeros_like(s))


# ---- (c) --------------------------------------------------------------------------------------------------------------
def wave_sum(vals):
    """Sum of up to-any-length f64 values the way one 64-lane wave forms it: lane-strided partials, then the xor-shuffle tree."""
    part = np.zeros(64, dtype=np.float64)
    for l, v in enumerate(vals):
        part[l % 64] += v
    for o in (32, 16, 8, 4, 2, 1):
        part = part + part[np.arange(64) ^ o]
    return float(part[0])


def pow_int(b, n):
    """b^n by the kernel's square-and-multiply, the same f64 products in the same order."""
    r = 1.0
    while n > 0:
        if n & 1:
            r *= b
        b *= b
        n >>= 1
    return r


class LatentAdam:
    """State and arithmetic of vg_latent_adam for B rows of L latents.  ``bf16``: dz / z_in / z_out are bf16 values."""

    def __init__(self, B, L, ZP, bf16=False):
        self.B, self.L, self.ZP, self.bf16 = B, L, ZP, bf16
        self.z = np.zeros((B, L), F32)
        self.m, self.v, self.best_z = self.z.copy(), self.z.copy(), self.z.copy()
        self.t = np.zeros(B, np.int32)
        self.best_loss = np.full(B, np.inf, F32)

    def _store(self, z):
        out = np.zeros((self.B, self.ZP), F32)
        out[:, :self.L] = bf16_round(z) if self.bf16 else z
        return out

    def init(self, z_in):
        z_in = np.asarray(z_in, F32).reshape(self.B, self.ZP)
        self.z = z_in[:, :self.L].copy()
        self.best_z = self.z.copy()
        self.m[:], self.v[:], self.t[:], self.best_loss[:] = 0, 0, 0, np.inf
        return self._store(self.z)

    def objective(self, loss_rows, p, alpha_adv, prior_weight):
        J = np.zeros(self.B, F32)
        for i in range(self.B):
            j = float(F32(loss_rows[i]))
            if p is not None:
                pi = float(F32(p[i]))
                logp = math.log(pi) if pi > 0 else (-math.inf if pi == 0 else math.nan)
                j += float(F32(alpha_adv)) * -max(logp, -100.0) if not math.isnan(logp) else math.nan
            if prior_weight != 0:
                q = wave_sum([float(zl) * float(zl) for zl in self.z[i]])
                j += float(F32(prior_weight)) * (q / (2.0 * self.L))
            J[i] = F32(j)
        return J

    def track(self, loss_rows, p=None, alpha_adv=0.0, prior_weight=0.0):
        J = self.objective(loss_rows, p, alpha_adv, prior_weight)
        for i in range(self.B):
            if J[i] < self.best_loss[i]:                # strict; False for a NaN
                self.best_loss[i] = J[i]
                self.best_z[i] = self.z[i]
        return J

    def update(self, dz, loss_rows, p=None, lr=0.05, betas=(0.9, 0.999), eps=1e-8, alpha_adv=0.0, prior_weight=0.0):
        J = self.track(loss_rows, p, alpha_adv, prior_weight)
        dz = np.asarray(dz, F32).reshape(self.B, self.ZP)
        b1, b2 = betas
        pw = float(F32(prior_weight))
        for i in range(self.B):
            tn = int(self.t[i]) + 1
            b1t, b2t = pow_int(b1, tn), pow_int(b2, tn)
            step_size, bc2_sqrt = lr / (1.0 - b1t), math.sqrt(1.0 - b2t)
            for l in range(self.L):
                zl = float(self.z[i, l])
                g = float(dz[i, l]) + pw * zl / float(self.L)
                mf = F32(b1 * float(self.m[i, l]) + (1.0 - b1) * g)
                vf = F32(b2 * float(self.v[i, l]) + (1.0 - b2) * g * g)
                self.z[i, l] = F32(zl - step_size * (float(mf) / (math.sqrt(float(vf)) / bc2_sqrt + eps)))
                self.m[i, l], self.v[i, l] = mf, vf
            self.t[i] = tn
        return J, self._store(self.z)


# ---- the loop ---------------------------------------------------------------------------------------------------------
WEIGHT_GAIN = 2.0       # on the N(0, 0.02) start: the pre-Tanh image then has a standard deviation near 1 (measured 1.0 at S = 16)


class Nets:
    """Reference-shaped Generator (+ Discriminator) states in f64 with non-trivial BatchNorm buffers, for eval-mode passes."""

    def __init__(self, S=16, L=100, seed=5, with_d=True):
        R.configure_seed(seed)
        self.S, self.L = S, L
        self.g_spec = R.generator_spec(nz=L, img_size=S)
        self.d_spec = R.discriminator_spec(img_size=S)
        self.G = R.make_sequential_state(self.g_spec)
        self.D = R.make_sequential_state(self.d_spec) if with_d else None
        R.weights_init_state(self.G, self.g_spec)
        if with_d:
            R.weights_init_state(self.D, self.d_spec)
        g = torch.Generator().manual_seed(seed + 1)
        for st in (self.G, self.D):
            if st is None:
                continue
            for k in list(st.keys()):
                # weights WEIGHT_GAIN times the N(0, 0.02) start, so that G(z) spans a good part of (-1, 1) and depends on z; buffers
                # as some training would leave them: means off zero, variances off one
                if k.endswith("running_mean"):
                    st[k] = 0.1 * torch.randn(st[k].shape, generator=g)
                elif k.endswith("running_var"):
                    st[k] = 0.5 + torch.rand(st[k].shape, generator=g)
                elif k.endswith(".bias"):
                    st[k] = 0.1 * torch.randn(st[k].shape, generator=g)
                elif k.endswith(".weight") and st[k].dim() == 4:
                    st[k] = st[k] * WEIGHT_GAIN
                if st[k].is_floating_point():
                    st[k] = st[k].detach().double()

    def decode(self, z):
        return R.generator_forward(self.G, self.g_spec, z[:, :, None, None], False)

    def discriminate(self, x):
        return R.discriminator_forward(self.D, self.d_spec, x, False)


def objective_terms(nets, z, noisy, rects, alpha_adv, prior_weight):
    """-> (J [B] the reported objective, T [B] the terms whose gradient the loop descends, loss_rows, p): J carries
    -max(log p, -100), T carries BCE(p, 0.9) -- the trainer's smoothed label -- in its place."""
    recon = nets.decode(z)
    loss = masked_mean_torch(recon, noisy, rects)
    prior = prior_weight * (z * z).sum(1) / (2.0 * z.shape[1])
    J, T, p = loss + prior, loss + prior, None
    if alpha_adv != 0.0:
        p = nets.discriminate(recon)
        J = J + alpha_adv * -torch.clamp(torch.log(p), min=-100.0)
        bce = -(REAL_LABEL * torch.clamp(torch.log(p), min=-100.0) + (1 - REAL_LABEL) * torch.clamp(torch.log(1 - p), min=-100.0))
        T = T + alpha_adv * bce
    return J, T, loss, p


def refine_loop(nets, noisy, rects, z0, steps, lr=0.05, betas=(0.9, 0.999), eps=1e-8, alpha_adv=0.0, prior_weight=0.0):
    """The refinement loop in f64: per row torch.optim.Adam's formulas on the gradient of T, keep-best on J.
    -> dict(z (last), best_z, best, objectives [steps + 1, B] (J at every iterate, the last one included), grads [steps, B, L])."""
    noisy, z = noisy.double(), z0.double().clone()
    B, L = z.shape
    m, v = torch.zeros_like(z), torch.zeros_like(z)
    best, best_z = torch.full((B,), math.inf, dtype=torch.float64), z.clone()
    objectives, grads = [], []
    b1, b2 = betas

    def keep(J, zc):
        nonlocal best, best_z
        better = J < best
        best = torch.where(better, J, best)
        best_z = torch.where(better[:, None], zc, best_z)

    for t in range(1, steps + 1):
        zr = z.clone().requires_grad_(True)
        J, T, _, _ = objective_terms(nets, zr, noisy, rects, alpha_adv, prior_weight)
        g, = torch.autograd.grad(T.sum(), zr)               # rows are independent in eval mode: row i gets dT_i / dz_i
        objectives.append(J.detach())
        grads.append(g)
        keep(J.detach(), z)
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        z = z - lr / (1 - b1 ** t) * m / (v.sqrt() / math.sqrt(1 - b2 ** t) + eps)
    with torch.no_grad():
        J, _, _, _ = objective_terms(nets, z, noisy, rects, alpha_adv, prior_weight)
    objectives.append(J)
    keep(J, z)
    return dict(z=z, best_z=best_z, best=best, objectives=torch.stack(objectives),
                grads=torch.stack(grads) if grads else torch.zeros(0, B, L, dtype=torch.float64))


# ---- the case of the refiner tests -----------------------------------------------------------------------------------
CASE_RECTS = [(5, 6, 3, 4), (4, 4, 10, 9), (7, 3, 0, 12), (3, 9, 6, 1)]     # rect_h, rect_w, x, y at S = 16
CASE_SEED = 40          # test_refine_cpu.py asserts the properties this seed was chosen for (steps = 5, lr = 0.05)
CASE_PRIOR = 0.01       # prior_weight of the refiner tests


def case_rects(B):
    out = torch.zeros(B, 8)
    for i in range(B):
        rh, rw, x, y = CASE_RECTS[i % len(CASE_RECTS)]
        out[i] = torch.tensor([0.5, 0.1, rh, rw, x, y, 0, 0], dtype=torch.float32)
    return out


def make_case(nets, B=4, seed=CASE_SEED, perturb=0.5):
    """-> (noisy f32 [B,3,S,S], rects f32 [B,8], z_star f32 [B,L], z0 f32 [B,L]): targets G(z*) with the rectangle painted
    a constant 1.0, the start z* + perturb * N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    z_star = torch.randn(B, nets.L, generator=g)
    z0 = (z_star + perturb * torch.randn(B, nets.L, generator=g)).float()
    with torch.no_grad():
        target = nets.decode(z_star.double()).float()
    rects = case_rects(B)
    noisy = torch.where(region_mask(rects, *target.shape), torch.ones_like(target), target)
    return noisy.contiguous(), rects, z_star.float(), z0
