"""Test infrastructure for the multi-scale SSIM loss (vg_msssim_loss_forward_backward, csrc/msssim.hip), CPU only: the
contract of include/vaegan_hip.h restated in torch, differentiable, in f64 (dtype=torch.float32 evaluates the same graph
in f32: the yardstick of the f32 cancellation in E[x^2] - E[x]^2, as in tests/_ssimloss_ref.py).

  default_weights        the default-scale rule of msssim_weights, written out independently of the package;
  pyramid                F.avg_pool2d(x, 2) levels;
  level_maps             cs and S over the interior of one level: the explicit 11 x 11 window with
                         tests/_pointwise_ref.gauss11, tap by tap;
  per_image_means        m_{b,j}: the cs mean of the levels below the last, the S mean of the last, per IMAGE;
  msssim_loss            1 - mean_b P_b with the clamp rule (P_b = 0 and no gradient when any m_{b,j} <= 0);
  loss_and_grad          value and gradient w.r.t. the first image through torch autograd;
  map_deviation          mean |map32_j - map64_j| per level (all images) and per (image, level);
  GPU_SHAPES, CLAMPED    the input table of tests/test_gpu_msssim.py and, per (shape, kind), the images the f64 restatement
                         puts on the clamp (tests/test_msssim_cpu.py asserts it, and that every |m_{b,j}| >= 1e-4);
  ref_step, ref_vae_step the iterations of tests/_ssimloss_ref.py with the structural term swapped.

Parity with the torchmetrics / pytorch-msssim packages is unpinned (neither is installed): the formulas are restated."""
from unittest import mock

import torch
import torch.nn.functional as F

import _pointwise_ref as P
import _ssimloss_ref as SR

U = P.U
C1, C2 = 0.01 ** 2, 0.03 ** 2
PAPER_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def default_scales(H, W):
    M = 0
    while M < 5 and (min(H, W) >> M) >= 11:
        M += 1
    return M


def default_weights(H, W, M=None):
    M = default_scales(H, W) if M is None else M
    s = sum(PAPER_WEIGHTS[:M])
    return tuple(w / s for w in PAPER_WEIGHTS[:M])


def pyramid(x, M):
    out = [x]
    for _ in range(M - 1):
        out.append(F.avg_pool2d(out[-1], 2))
    return out


def level_maps(a, b, dtype=torch.float64):
    """-> (cs, S) over the interior pixels of one level, [B, C, H - 10, W - 10]; a, b in [-1, 1]."""
    a = (a.to(dtype) + 1) * 0.5
    b = (b.to(dtype) + 1) * 0.5
    g = P.gauss11(dtype)
    H, W = a.shape[-2:]
    IH, IW = H - 10, W - 10
    z = torch.zeros(a.shape[:2] + (IH, IW), dtype=dtype)
    ma, mb, saa, sbb, sab = z.clone(), z.clone(), z.clone(), z.clone(), z.clone()
    for dy in range(11):
        for dx in range(11):
            w = g[dy] * g[dx]
            va, vb = a[..., dy:dy + IH, dx:dx + IW], b[..., dy:dy + IH, dx:dx + IW]
            ma = ma + w * va
            mb = mb + w * vb
            saa = saa + w * va * va
            sbb = sbb + w * vb * vb
            sab = sab + w * va * vb
    vaa, vbb, vab = saa - ma * ma, sbb - mb * mb, sab - ma * mb
    cs = (2 * vab + C2) / (vaa + vbb + C2)
    return cs, ((2 * ma * mb + C1) / (ma * ma + mb * mb + C1)) * cs


def all_maps(a, b, M, dtype=torch.float64):
    """The map every level contributes: cs below the last level, S at it."""
    pa, pb = pyramid(a.to(dtype), M), pyramid(b.to(dtype), M)
    return [level_maps(pa[j], pb[j], dtype)[0 if j < M - 1 else 1] for j in range(M)]


def per_image_means(a, b, M, dtype=torch.float64):
    """-> [B, M] (differentiable)."""
    return torch.stack([m.mean(dim=(1, 2, 3)) for m in all_maps(a, b, M, dtype)], dim=1)


def products(m, weights):
    """P_b of the means [B, M]: prod_j m^{w_j} where every m_{b,j} > 0, else 0 with no gradient."""
    ok = (m > 0).all(dim=1)
    w = torch.tensor(weights, dtype=m.dtype)
    safe = torch.where(ok[:, None], m, torch.ones_like(m))
    return torch.where(ok, (safe ** w).prod(dim=1), torch.zeros_like(safe[:, 0]))


def msssim_loss(a, b, weights, dtype=torch.float64):
    return 1.0 - products(per_image_means(a, b, len(weights), dtype), weights).mean()


def loss_and_grad(a, b, weights, dtype=torch.float64):
    """-> (loss, d loss / d a, m [B, M]) as f64 tensors, evaluated in `dtype` by torch autograd.  b is a constant."""
    x = a.detach().to(dtype).clone().requires_grad_(True)
    m = per_image_means(x, b.detach().to(dtype), len(weights), dtype)
    loss = 1.0 - products(m, weights).mean()
    if loss.requires_grad and bool((m > 0).all(dim=1).any()):
        (g,) = torch.autograd.grad(loss, x)
    else:
        g = torch.zeros_like(x)            # every image on the clamp: the graph does not reach x
    return loss.detach().double(), g.double(), m.detach().double()


def map_deviation(a, b, M):
    """-> (mean |map32_j - map64_j| per level [M], the same per (image, level) [B, M])."""
    m32, m64 = all_maps(a, b, M, torch.float32), all_maps(a, b, M)
    dev = [(x.double() - y).abs() for x, y in zip(m32, m64)]
    return torch.stack([d.mean() for d in dev]), torch.stack([d.mean(dim=(1, 2, 3)) for d in dev], dim=1)


# ---- the input table of tests/test_gpu_msssim.py ---------------------------------------------------------------------
GPU_SHAPES = [((1, 1, 22, 22), 2),         # the coarse level is one interior pixel
              ((2, 3, 23, 37), 2),         # odd both ways: a dropped row and a dropped column
              ((2, 3, 64, 64), 3),         # the project's plane
              ((1, 3, 70, 45), 3),         # ragged tiles, last level 17 x 11
              ((1, 1, 11, 300), 1),        # single scale
              ((1, 1, 176, 176), 5),       # the smallest five-scale plane
              ((2, 1, 256, 256), 5)]       # the 256 geometry
MIN_ABS_MEAN = 1e-4                        # every |m_{b,j}| of the table: two orders above what an f32 mean can move
# (shape, kind) -> the images the f64 restatement puts on the clamp; pairs not listed have none.
CLAMPED = {}
for _shape, _ in GPU_SHAPES:
    CLAMPED[(_shape, "negated")] = tuple(range(_shape[0]))
for _shape in ((2, 3, 23, 37), (1, 3, 70, 45), (1, 1, 11, 300), (1, 1, 176, 176)):
    CLAMPED[(_shape, "noise")] = tuple(range(_shape[0]))
CLAMPED[((2, 3, 64, 64), "noise")] = (0,)          # the mixed cases: one image on the clamp, one not
CLAMPED[((2, 1, 256, 256), "noise")] = (1,)        # (its m_{1,4} = -5.5e-4 is the smallest |m| of the table)


def clamped(shape, kind):
    return CLAMPED.get((tuple(shape), kind), ())


# ---- the iterations --------------------------------------------------------------------------------------------------
def _swapped(weights):
    """_ssimloss_ref's structural term replaced by the multi-scale one for the duration of a step."""
    return mock.patch.object(SR, "ssim_loss", lambda a, b, dtype=torch.float64: msssim_loss(a, b, weights, dtype))


def ref_step(model, real, eps_z, eps_real, eps_recon, epoch, ssim_scales=None, **kw):
    """_ssimloss_ref.ref_step; with ssim_scales (a weight tuple) the term is alpha_ssim (1 - MS-SSIM(recon, real))."""
    if ssim_scales is None:
        return SR.ref_step(model, real, eps_z, eps_real, eps_recon, epoch, **kw)
    with _swapped(tuple(ssim_scales)):
        return SR.ref_step(model, real, eps_z, eps_real, eps_recon, epoch, **kw)


def ref_vae_step(model, img, eps_img, eps_z, epoch, ssim_scales=None, **kw):
    if ssim_scales is None:
        return SR.ref_vae_step(model, img, eps_img, eps_z, epoch, **kw)
    with _swapped(tuple(ssim_scales)):
        return SR.ref_vae_step(model, img, eps_img, eps_z, epoch, **kw)
