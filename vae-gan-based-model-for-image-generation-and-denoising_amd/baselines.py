"""Classical-denoiser baselines for the denoising passes (not in the reference): what a parameter-free filter reaches on the
same pairs, so that ``psnr`` next to ``psnr_noisy`` can be read.  All compute is HIP kernels (csrc/nlm.hip)."""
import math
from typing import Optional

import torch

from . import ops


DEFAULT_H_FACTOR = 0.8          # h = 0.8 sigma: the dB table behind it is in DESIGN.md section 4.4r (tools/nlm_bench.py)


class NLMeans:
    """Non-local means (Buades, Coll & Morel 2005; ``ops.nlm_denoise``): pixelwise, uniform (2P+1)^2 patch, (2R+1)^2 search
    window, weight exp(-max(d2 - 2 sigma^2, 0) / h^2) with h = h_factor * sigma per image.  It has no weights; its one
    parameter is the noise level ``sigma``:

        "oracle"    the level the degraded loader drew for each image: column 1 of ``rects`` (``DeviceLoader.last_rects``,
                    ops.degrade_params' layout), read in place;
        "estimate"  Immerkaer's blind estimate of each noisy image (``ops.noise_sigma``);
        a number    that level for every image (> 0, in the units of the images).

    ``__call__(noisy, rects=None)`` -> f32 [B,C,H,W]; noisy: f32 [B,C,H,W] on the MI355X, C <= 4, min(H, W) >= P + R + 1.
    Two launches at most, no host synchronisation.  An image whose level is 0 (or not finite) comes back unchanged."""

    name = "nlm"

    def __init__(self, patch_radius: int = 2, search_radius: int = 7, h_factor: float = DEFAULT_H_FACTOR, sigma="oracle"):
        for name, v, lo, hi in (("patch_radius", patch_radius, 0, 3), ("search_radius", search_radius, 1, 10)):
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
                raise ValueError(f"{name} must be an integer in {lo}..{hi}")
        if isinstance(h_factor, bool) or not isinstance(h_factor, (int, float)) or not (math.isfinite(h_factor) and h_factor > 0):
            raise ValueError("h_factor must be finite and > 0")
        if isinstance(sigma, str):
            if sigma not in ("oracle", "estimate"):
                raise ValueError(f"sigma must be 'oracle', 'estimate' or a number > 0, got {sigma!r}")
        elif isinstance(sigma, bool) or not isinstance(sigma, (int, float)) or not (math.isfinite(sigma) and sigma > 0):
            raise ValueError("sigma must be 'oracle', 'estimate' or a finite number > 0")
        self.patch_radius, self.search_radius, self.h_factor = patch_radius, search_radius, float(h_factor)
        self.sigma = sigma if isinstance(sigma, str) else float(sigma)

    @property
    def needs_rects(self) -> bool:
        return self.sigma == "oracle"

    @torch.no_grad()
    def __call__(self, noisy: torch.Tensor, rects: Optional[torch.Tensor] = None) -> torch.Tensor:
        what = "NLMeans"
        if not isinstance(noisy, torch.Tensor) or not noisy.is_cuda:
            raise RuntimeError(f"{what} needs the batch on the MI355X ('cuda'); there is no CPU path")
        if noisy.dim() != 4 or noisy.dtype != torch.float32:
            raise RuntimeError(f"{what}: noisy must be float32 [B,C,H,W]")
        noisy = noisy.contiguous()
        B = noisy.shape[0]
        if self.sigma == "oracle":
            if rects is None or not rects.is_cuda or rects.dtype != torch.float32 or tuple(rects.shape) != (B, 8):
                raise RuntimeError(f"{what}: sigma='oracle' needs rects, the device f32 [B, 8] tensor of ops.degrade_params "
                                   f"(DeviceLoader.last_rects)")
            sigma = rects[:, 1]
        elif self.sigma == "estimate":
            sigma = ops.noise_sigma(noisy)
        else:
            sigma = self.sigma
        return ops.nlm_denoise(noisy, sigma, patch_radius=self.patch_radius, search_radius=self.search_radius,
                               h_factor=self.h_factor)


class Median:
    """Median filter (``ops.median_filter``): the per-channel (2r+1)^2 median, r = radius in {1, 2}, reflect padding -- the
    textbook baseline under impulse noise (salt and pepper), where a Gaussian sigma tells non-local means nothing.  It has no
    noise-level parameter and reads no rectangles.

    ``__call__(noisy, rects=None)`` -> f32 [B,C,H,W]; noisy: f32 [B,C,H,W] on the MI355X, min(H, W) >= radius + 1.  One launch,
    no host synchronisation."""

    name = "median"
    needs_rects = False

    def __init__(self, radius: int = 1):
        if isinstance(radius, bool) or not isinstance(radius, int) or not 1 <= radius <= 2:
            raise ValueError(f"radius must be an integer in 1..2, got {radius!r}")
        self.radius = radius

    @torch.no_grad()
    def __call__(self, noisy: torch.Tensor, rects: Optional[torch.Tensor] = None) -> torch.Tensor:
        what = "Median"
        if not isinstance(noisy, torch.Tensor) or not noisy.is_cuda:
            raise RuntimeError(f"{what} needs the batch on the MI355X ('cuda'); there is no CPU path")
        if noisy.dim() != 4 or noisy.dtype != torch.float32:
            raise RuntimeError(f"{what}: noisy must be float32 [B,C,H,W]")
        return ops.median_filter(noisy.contiguous(), self.radius)


_ACCEPTS = "None, an NLMeans, a Median, 'nlm', 'median' or a dict of NLMeans' keywords or with the key 'radius'"


def make_baseline(what: str, baseline, allow_oracle: bool = True):
    """``baseline=`` of the evaluation passes: None, an NLMeans or a Median, the string "nlm" or "median", or a dict -- of
    NLMeans' keywords, or ``{"radius": r}`` for a Median.  The result's ``name`` suffixes the result keys."""
    if baseline is None:
        return None
    if isinstance(baseline, (NLMeans, Median)):
        made = baseline
    elif isinstance(baseline, str):
        if baseline == "median":
            made = Median()
        elif baseline == "nlm":
            made = NLMeans() if allow_oracle else NLMeans(sigma="estimate")
        else:
            raise ValueError(f"{what}: baseline must be {_ACCEPTS}, got {baseline!r}")
    elif isinstance(baseline, dict):
        try:
            made = Median(**baseline) if "radius" in baseline else NLMeans(**baseline)
        except TypeError as e:
            raise ValueError(f"{what}: baseline: {e}") from None
    else:
        raise ValueError(f"{what}: baseline must be {_ACCEPTS}")
    if made.needs_rects and not allow_oracle:
        raise ValueError(f"{what}: there is no loader whose noise levels could be read: the baseline needs sigma='estimate' "
                         f"or a number")
    return made


def check_oracle_sigma(what: str, baseline, loader) -> None:
    """sigma="oracle" reads column 1 of the loader's rectangle records as the standard deviation of additive Gaussian noise.
    Under any other noise model of the loader's ``Degrade`` that column is not one: refuse instead of filtering with it."""
    degrade = getattr(loader, "degrade", None)
    if isinstance(baseline, NLMeans) and baseline.sigma == "oracle" and degrade is not None and not degrade.pure_gaussian:
        raise ValueError(f"{what}: the loader degrades with {degrade!r}; column 1 of its rectangle records (s * noise_max_std) "
                         f"is then not a Gaussian sigma, which NLMeans(sigma='oracle') takes it for: use sigma='estimate' or "
                         f"a number")
