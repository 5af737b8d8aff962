"""f64 torch (CPU) restatements of the pointwise, loss and SSIM entry points, straight from their contracts in
include/vaegan_hip.h: the yardstick of tests/test_pointwise_cpu.py and tests/test_gpu_pointwise.py.  One small function
per entry point, written for reading, nothing here calls the package.  Inputs are taken as given (the tests round them to
the storage dtype first) and promoted to f64; f32 scalar arguments (targets, sigma, gscale ...) are rounded to f32 first,
because that is the number the C ABI receives.

The second half holds the seeded input generators of the GPU tests, with the conditions that keep a test from passing
vacuously (asserted in test_pointwise_cpu.py)."""
import numpy as np
import torch

U = 2.0 ** -24          # unit roundoff of f32 (round to nearest)
UB = 2.0 ** -8          # unit roundoff of bf16: 8 significant bits, so round-to-nearest errs by up to 2^-8 |x| (2^-9 |x| is
                        # missed by the correctly rounded conversion itself: test_pointwise_cpu.py shows it)
# HIP's documented bounds (HIP math API, single precision): expf 1 ulp, logf 1 ulp, tanhf 2 ulp; 1 ulp <= 2 U relative
EXP_U, LOG_U, TANH_U = 2, 2, 4


def f32(v):
    """A python scalar as the f32 the C ABI receives, back as a python float."""
    return float(np.float32(v))


def d(t):
    return t.detach().to(torch.float64)


# ---- layout family -----------------------------------------------------------------------------------------------------
def to_nhwc(x, CP):
    """NCHW -> NHWC with the channels padded to CP by zeros."""
    B, C, H, W = x.shape
    y = torch.zeros(B, H, W, CP, dtype=x.dtype)
    y[..., :C] = x.permute(0, 2, 3, 1)
    return y


def from_nhwc(y, C):
    return y[..., :C].permute(0, 3, 1, 2).contiguous()


def nchw_to_nhwc(x, CP, eps=None, sigma=0.0):
    """vg_nchw_to_nhwc: y = x (+ sigma * eps), NHWC, pad channels zero."""
    v = d(x) if eps is None else d(x) + f32(sigma) * d(eps)
    return to_nhwc(v, CP)


def noisy_clamp_to_nhwc(x, eps, sigma, lo, hi, CP):
    """vg_noisy_clamp_to_nhwc -> (NHWC, NCHW): clamp(x + sigma * eps, lo, hi)."""
    v = torch.clamp(d(x) + f32(sigma) * d(eps), f32(lo), f32(hi))
    return to_nhwc(v, CP), v


def nhwc_to_nchw(y, C, apply_tanh=False):
    v = from_nhwc(d(y), C)
    return torch.tanh(v) if apply_tanh else v


def nhwc_tanh_to_nchw_noisy(y, C, eps, sigma):
    """vg_nhwc_tanh_to_nchw_noisy -> (tanh(x) NCHW, tanh(x) + sigma * eps NHWC padded like y)."""
    t = torch.tanh(from_nhwc(d(y), C))
    return t, to_nhwc(t + f32(sigma) * d(eps), y.shape[-1])


def nchw_grad_to_nhwc(dy, CP, tanh_out=None, add_nhwc=None):
    """vg_nchw_grad_to_nhwc / vg_nchw_grad_add_to_nhwc: dx = (dy [+ add]) [* (1 - t^2)], NHWC."""
    v = d(dy)
    if add_nhwc is not None:
        v = v + from_nhwc(d(add_nhwc), dy.shape[1])
    if tanh_out is not None:
        v = v * (1.0 - d(tanh_out) ** 2)
    return to_nhwc(v, CP)


# ---- reparameterisation / KL -------------------------------------------------------------------------------------------
def reparam_forward(mulv, eps, L, ZP):
    """-> (z [B, ZP] with pad 0, lv_clamped [B, L])."""
    m = d(mulv)
    mu, lv = m[:, :L], torch.clamp(m[:, L:2 * L], -10.0, 10.0)
    z = torch.zeros(m.shape[0], ZP, dtype=torch.float64)
    z[:, :L] = mu + torch.exp(0.5 * lv) * d(eps)
    return z, lv


def kl_forward(mulv, L, divisor):
    m = d(mulv)
    mu, lv = m[:, :L], torch.clamp(m[:, L:2 * L], -10.0, 10.0)
    return -0.5 * torch.sum(1.0 + lv - mu * mu - torch.exp(lv)) / f32(divisor)


def kl_abs_terms(mulv, L):
    """sum_i (1 + |lv| + mu^2 + exp(lv)): the magnitudes an f32 evaluation of one KL term passes through."""
    m = d(mulv)
    mu, lv = m[:, :L], torch.clamp(m[:, L:2 * L], -10.0, 10.0)
    return torch.sum(1.0 + lv.abs() + mu * mu + torch.exp(lv))


def reparam_kl_backward(mulv, eps, dz, kl_scale, L):
    """-> dmulv [B, MP]: d mu = dz + ks mu;  d logvar = [raw in [-10, 10]] (dz .5 exp(.5 lv) eps + ks .5 (exp(lv) - 1));
    pad columns zero.  dz: [B, ZP]."""
    m, ks = d(mulv), f32(kl_scale)
    B, MP = m.shape
    mu, raw = m[:, :L], m[:, L:2 * L]
    lv = torch.clamp(raw, -10.0, 10.0)
    g = d(dz)[:, :L]
    out = torch.zeros(B, MP, dtype=torch.float64)
    out[:, :L] = g + ks * mu
    passes = (raw >= -10.0) & (raw <= 10.0)
    out[:, L:2 * L] = torch.where(passes, g * 0.5 * torch.exp(0.5 * lv) * d(eps) + ks * 0.5 * (torch.exp(lv) - 1.0),
                                  torch.zeros((), dtype=torch.float64))
    return out


def reparam_kl_backward_mag(mulv, eps, dz, kl_scale, L):
    """Magnitudes the f32 evaluation passes through, per output element (for the error bound)."""
    m, ks = d(mulv), abs(f32(kl_scale))
    B, MP = m.shape
    mu, lv = m[:, :L], torch.clamp(m[:, L:2 * L], -10.0, 10.0)
    g = d(dz)[:, :L].abs()
    out = torch.zeros(B, MP, dtype=torch.float64)
    out[:, :L] = g + ks * mu.abs()
    out[:, L:2 * L] = g * 0.5 * torch.exp(0.5 * lv) * d(eps).abs() + ks * 0.5 * (torch.exp(lv) + 1.0)
    return out


# ---- Discriminator head --------------------------------------------------------------------------------------------------
def dot_sigmoid_forward(x, w):
    """x [B, K], w [K] -> (p [B], sum_k |x w| [B])."""
    prod = d(x) * d(w)[None, :]
    return torch.sigmoid(prod.sum(1)), prod.abs().sum(1)


def dot_sigmoid_backward(p, dp, w):
    """-> (dlogit [B] = dp p (1 - p), dx [B, K] = dlogit w)."""
    dl = d(dp) * d(p) * (1.0 - d(p))
    return dl, dl[:, None] * d(w)[None, :]


def dot_wgrad(x, dlogit, C, HW):
    """dw[c][hw] = sum_b dlogit[b] x[b, hw * C + c] (x NHWC-flattened, dw in the [1][C][kh][kw] layout)
    -> (dw [C, HW], sum_b |dlogit x| [C, HW])."""
    prod = d(dlogit)[:, None] * d(x)
    lay = lambda v: v.view(HW, C).t().contiguous()
    return lay(prod.sum(0)), lay(prod.abs().sum(0))


def bce_terms(p, target):
    """-(t max(log p, -100) + (1 - t) max(log(1 - p), -100)) per sample (nn.BCELoss) -> (terms, magnitudes)."""
    p, t = d(p), f32(target)
    l1 = torch.clamp(torch.log(p), min=-100.0)
    l2 = torch.clamp(torch.log1p(-p), min=-100.0)
    return -(t * l1 + (1.0 - t) * l2), t * l1.abs() + (1.0 - t) * (l2.abs() + 1.0)


def bce(p, target):
    return bce_terms(p, target)[0].mean()


def bce_grad(p, target, gscale):
    """dp = gscale (p - t) / max(p (1 - p), 1e-12) / B."""
    p = d(p)
    return f32(gscale) * (p - f32(target)) / torch.clamp(p * (1.0 - p), min=f32(1e-12)) / p.numel()


def head_backward(p, x, w, B, groups, t0, t1, gscale, C, HW):
    """vg_head_backward -> dict(loss, dlogit [R], dx [R, K], dw [C, HW], dw_abs [C, HW]); p [groups * B]."""
    p = d(p)
    loss = bce(p[:B], t0) + (bce(p[B:], t1) if groups == 2 else 0.0)
    dp = torch.cat([bce_grad(p[:B], t0, gscale)] + ([bce_grad(p[B:], t1, gscale)] if groups == 2 else []))
    dl, dx = dot_sigmoid_backward(p, dp, w)
    dw, dw_abs = dot_wgrad(x, dl, C, HW)
    return dict(loss=loss, dlogit=dl, dx=dx, dw=dw, dw_abs=dw_abs)


# ---- losses, clamp, axpy ---------------------------------------------------------------------------------------------------
def mean_loss(p, sign):
    return f32(sign) * d(p).mean()


def mean_grad(p, sign, gscale):
    return torch.full((p.numel(),), f32(sign) * f32(gscale) / p.numel(), dtype=torch.float64)


def mse(a, b):
    return ((d(a) - d(b)) ** 2).mean()


def mse_grad(a, b, gscale):
    return f32(gscale) * 2.0 * (d(a) - d(b)) / a.numel()


def clamp_f32(x, lo, hi):
    """vg_clamp, as the f32 torch expression (no rounding happens: the result is one of three f32 numbers)."""
    return torch.clamp(x.float(), f32(lo), f32(hi))


def axpy_f32(a, b, alpha):
    """vg_axpy as the f32 torch expression a + alpha * b (product rounded, then the sum)."""
    return a.float() + torch.tensor(alpha, dtype=torch.float32) * b.float()


# ---- bn_act.hip neighbours ---------------------------------------------------------------------------------------------------
def act_backward(x, dy, act, slope):
    """act 1: ReLU, 2: LeakyReLU(slope).  dx = dy where x > 0, else 0 / dy * slope."""
    x, dy = d(x), d(dy)
    return torch.where(x > 0, dy, dy * (f32(slope) if act == 2 else 0.0))


def bias_grad(dy, NC):
    """dy [rows, C] -> (column sums [NC], sum of magnitudes [NC])."""
    return d(dy)[:, :NC].sum(0), d(dy)[:, :NC].abs().sum(0)


# ---- SSIM ------------------------------------------------------------------------------------------------------------------
def gauss11(dtype=torch.float64):
    k = torch.arange(11, dtype=dtype) - 5
    g = torch.exp(-(k * k) / (2 * 1.5 * 1.5))
    return g / g.sum()


def ssim_map(a, b, dtype=torch.float64):
    """Per interior pixel (5-pixel border dropped, so no padding is ever read), the explicit 11x11 Gaussian window, tap by
    tap: a, b NCHW in [-1, 1], rescaled to [0, 1] -> the SSIM map [B, C, H - 10, W - 10].  dtype=torch.float32 evaluates
    the same formula in f32 on the CPU (the yardstick of the kernel's f32 cancellation in E[x^2] - E[x]^2)."""
    a = (a.to(dtype) + 1) * 0.5
    b = (b.to(dtype) + 1) * 0.5
    g = gauss11(dtype)
    H, W = a.shape[-2:]
    IH, IW = H - 10, W - 10
    z = torch.zeros(a.shape[:2] + (IH, IW), dtype=dtype)
    ma, mb, saa, sbb, sab = z.clone(), z.clone(), z.clone(), z.clone(), z.clone()
    for dy in range(11):
        for dx in range(11):
            w = g[dy] * g[dx]
            va, vb = a[..., dy:dy + IH, dx:dx + IW], b[..., dy:dy + IH, dx:dx + IW]
            ma += w * va
            mb += w * vb
            saa += w * va * va
            sbb += w * vb * vb
            sab += w * va * vb
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    vaa, vbb, vab = saa - ma * ma, sbb - mb * mb, sab - ma * mb
    return ((2 * ma * mb + c1) * (2 * vab + c2)) / ((ma * ma + mb * mb + c1) * (vaa + vbb + c2))


def ssim(a, b):
    return float(ssim_map(a, b).mean())


# ---- input generators of tests/test_gpu_pointwise.py ---------------------------------------------------------------------------
def q(t, bf16):
    """Round to the storage dtype the kernel sees, back in f64 (so that the reference isolates the kernel's error)."""
    return t.to(torch.bfloat16).double() if bf16 else t.float().double()


def gen(seed):
    return torch.Generator().manual_seed(seed)


def reparam_inputs(B, L, MP, ZP, bf16, seed=0):
    """-> mulv [B, MP] (pad columns hold junk the kernels must not use), eps [B, L] f32, dz [B, ZP] (pad junk).
    logvar ~ N(0, 10^2): about 32 % outside [-10, 10]; a handful sits exactly on +-10 (inclusive gradient mask)."""
    g = gen(1000 * B + L + MP + seed)
    mulv = torch.randn(B, MP, generator=g)
    mulv[:, L:2 * L] *= 10.0
    lv = mulv[:, L:2 * L].reshape(-1)
    pick = torch.randperm(lv.numel(), generator=g)[:4]
    lv[pick] = torch.tensor([10.0, -10.0, 10.0, -10.0])[:pick.numel()]
    mulv[:, L:2 * L] = lv.view(B, L)
    eps = torch.randn(B, L, generator=g)
    dz = torch.randn(B, ZP, generator=g)
    return q(mulv, bf16), eps.double(), q(dz, bf16)


def noisy_clamp_inputs(B, C, H, W, seed=0):
    """x ~ N(0, 1.2^2), eps ~ N(0, 1), sigma 0.5: x + sigma eps has deviation 1.3, about 22 % beyond each of -1, 1."""
    g = gen(77 + B + C + H + W + seed)
    return (torch.randn(B, C, H, W, generator=g) * 1.2).double(), torch.randn(B, C, H, W, generator=g).double(), 0.5


def act_inputs(n, bf16, seed=0):
    """x with half the signs negative (shuffled) and |x| in [0.01, 2]: no value near the branch point, after storage
    rounding either."""
    g = gen(31 + n + seed)
    mag = 0.01 + 1.99 * torch.rand(n, generator=g)
    sign = torch.ones(n)
    sign[::2] = -1.0
    sign = sign[torch.randperm(n, generator=g)]
    return q(mag * sign, bf16), q(torch.randn(n, generator=g), bf16)


def bce_probs(B, seed=0):
    """p in (0, 1) from a logistic of N(0, 2^2), with exact 0 and 1 and neighbours within 1e-7 of both planted first."""
    g = gen(5 + B + seed)
    p = torch.sigmoid(torch.randn(B, generator=g) * 2).float()
    edge = torch.tensor([0.0, 1.0, 1e-7, 1.0 - 2.0 ** -24, 3e-8, 1.0 - 2.0 ** -23], dtype=torch.float32)
    idx = torch.randperm(B, generator=g)[:min(B, edge.numel())]
    p[idx] = edge[:idx.numel()]
    return p.double()


SSIM_KINDS = ("noise", "same", "negated", "small_noise", "constant", "blocks")


def ssim_inputs(kind, B, C, H, W, seed=0):
    g = gen(900 + B + C + H + W + seed)
    u = lambda: torch.rand(B, C, H, W, generator=g) * 2 - 1
    if kind == "noise":
        return u(), u()
    if kind == "same":
        a = u()
        return a, a.clone()
    if kind == "negated":
        a = u()
        return a, -a
    if kind == "small_noise":                          # a smooth image (low-pass noise) plus N(0, 0.1^2)
        yy = torch.linspace(0, 3.0, H)[:, None] + torch.rand(B, C, 1, 1, generator=g) * 6
        xx = torch.linspace(0, 2.0, W)[None, :] + torch.rand(B, C, 1, 1, generator=g) * 6
        a = 0.8 * torch.sin(yy) * torch.cos(xx)
        return a, torch.clamp(a + 0.1 * torch.randn(B, C, H, W, generator=g), -1, 1)
    if kind == "constant":
        return torch.full((B, C, H, W), 0.3), torch.full((B, C, H, W), -0.2)
    if kind == "blocks":                                # piecewise constant 4x4 blocks, b shifted by one pixel
        cells = torch.rand(B, C, (H + 3) // 4 + 1, (W + 3) // 4 + 1, generator=g) * 2 - 1
        big = cells.repeat_interleave(4, -2).repeat_interleave(4, -1)
        return big[..., :H, :W].contiguous(), big[..., 1:H + 1, 1:W + 1].contiguous()
    raise ValueError(kind)
