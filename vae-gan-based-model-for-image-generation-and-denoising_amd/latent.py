"""Generation path of the reference: the aggregate-posterior histogram prior and the generation evaluation
(main_vae.py:415-436 vals_to_hist / sample_distribution, :438-512 evaluate_vae, :514-575 eval_vae, :577-641 sample_vae,
:348-374 sample_vae_decoder, and the per-epoch ``decoder(fixed_noise)`` picture of vaegan_code.py:209-216).

The reference's better sampler does not draw z ~ N(0, I): it runs the eval-mode Encoder over the WHOLE data set, keeps
every mu and logvar, fits a 100-bin histogram per latent dimension and draws mu and logvar by inverse-CDF sampling before
it reparameterises and decodes.  Here the Encoder's outputs never leave the device: ``encode_dataset`` writes them into
one [N, 2L] buffer, ``LatentPrior.fit`` fits the 2L histograms with one HIP call (vg_latent_hist), ``sample_z`` draws
straight into the Generator's input layout (vg_latent_sample) and ``sample_images`` / ``evaluate_generation`` decode and
score.  The contracts -- f32 edges as numpy >= 2 computes them, the f64 cdf summed in bin order, the two stated
deviations -- are in include/vaegan_hip.h, "Latent prior".  All compute is HIP kernels.  FID and precision / recall / F1
are computed in the feature space of a pluggable ``feature_fn`` (metrics.py; the project's own Encoder by default);
InceptionV3 itself needs downloaded weights, so Inception Score is out of scope.
"""
from typing import Dict, Iterable, Optional, Tuple

import torch

from . import geometry as G
from . import ops
from .metrics import FeaturePass, _pr_result


def _loader_samples(loader) -> int:
    """Images one pass over the loader yields (len(loader.dataset) of the reference's DataLoader over a Subset)."""
    if hasattr(loader, "global_batches") and hasattr(loader, "indices"):
        return sum(hi - lo for lo, hi in loader.global_batches(loader.indices.numel()))
    return len(loader.dataset)


@torch.no_grad()
def encode_dataset(encoder, *loaders) -> Tuple[torch.Tensor, int]:
    """main_vae.py:452-467: ``encoder.eval()``, one pass over every loader (data.DeviceLoader yielding clean batches, the
    ragged last batch included), in the order given.  -> (mulv, n): mulv f32 [N, 2L] on the device, row k = the fused
    ``mu | logvar`` of the k-th image seen, the values of ``encoder(batch)`` in eval mode, NOT clamped (:458);
    n = N = the images seen.  The buffer is allocated once; there is no host sync inside the pass."""
    if not loaders:
        raise RuntimeError("encode_dataset needs at least one loader")
    encoder.eval()                                                                   # :452
    dev = next(encoder.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError("encode_dataset needs the Encoder on the MI355X ('cuda'); there is no CPU path")
    L2 = 2 * encoder.latent_dim
    N = sum(_loader_samples(ld) for ld in loaders)
    if N < 1:
        raise RuntimeError("encode_dataset: the loaders hold no image")
    out = torch.empty(N, L2, dtype=torch.float32, device=dev)
    k = 0
    for ld in loaders:
        for img in ld:
            if isinstance(img, (tuple, list)):
                raise RuntimeError("encode_dataset needs clean batches, this loader yields (noisy, clean) pairs")
            if not img.is_cuda:
                raise RuntimeError("encode_dataset needs device batches (data.DeviceLoader); there is no CPU path")
            b = img.shape[0]
            if k + b > N:
                raise RuntimeError("encode_dataset: a loader yielded more images than it announced")
            mulv, _ = encoder.engine_forward(img, keep=False)                        # [b, MP] engine dtype
            out[k:k + b].copy_(mulv[:, :L2])                                         # widening copy of the 2L real columns
            k += b
    if k != N:
        raise RuntimeError(f"encode_dataset: the loaders announced {N} images and yielded {k}")
    return out, N


class LatentPrior:
    """The fitted histogram prior of main_vae.py:469-470 (mu_bins / mu_cdfs and logvar_bins / logvar_cdfs as ONE set of
    2L columns: [0, L) mu, [L, 2L) logvar).  Device tensors: ``edges`` f32 [2L, n_bins+1], ``counts`` int32 [2L, n_bins],
    ``cdf`` f64 [2L, n_bins]; ``n_fitted`` rows went in."""

    def __init__(self, edges: torch.Tensor, counts: torch.Tensor, cdf: torch.Tensor, latent_dim: int, n_fitted: int):
        for t in (edges, counts, cdf):
            if not t.is_cuda:
                raise RuntimeError("LatentPrior lives on the MI355X ('cuda'); there is no CPU path")
        L, nb = int(latent_dim), cdf.shape[-1]
        if (tuple(edges.shape) != (2 * L, nb + 1) or tuple(counts.shape) != (2 * L, nb) or tuple(cdf.shape) != (2 * L, nb)
                or edges.dtype != torch.float32 or counts.dtype != torch.int32 or cdf.dtype != torch.float64):
            raise RuntimeError("LatentPrior: edges f32 [2L,n_bins+1], counts int32 [2L,n_bins], cdf f64 [2L,n_bins]")
        self.edges, self.counts, self.cdf = edges.contiguous(), counts.contiguous(), cdf.contiguous()
        self.latent_dim, self.n_bins, self.n_fitted = L, nb, int(n_fitted)

    @classmethod
    def fit(cls, mulv: torch.Tensor, latent_dim: int, n_bins: int = 100) -> "LatentPrior":
        """vals_to_hist (main_vae.py:415-425) of the mu and of the logvar columns in one call.  mulv: f32 [N, 2L] on the
        device (encode_dataset).  Raises RuntimeError where numpy raises ValueError: a column whose range is not finite.
        ONE host sync (the status word)."""
        if not mulv.is_cuda:
            raise RuntimeError("LatentPrior.fit needs the latents on the MI355X ('cuda'); there is no CPU path")
        if mulv.dim() != 2 or mulv.shape[1] != 2 * int(latent_dim):
            raise RuntimeError(f"LatentPrior.fit: mulv must be [N, {2 * int(latent_dim)}] (mu | logvar)")
        edges, counts, cdf, status = ops.latent_hist(mulv, n_bins)
        if int(status.item()) != 0:
            raise RuntimeError("LatentPrior.fit: a latent column holds a NaN or an infinity (its range is not finite)")
        return cls(edges, counts, cdf, latent_dim, mulv.shape[0])

    def _draws(self, u, v, need_state: bool):
        if (u is None) != (v is None):
            raise RuntimeError("LatentPrior: inject both u and v, or neither")
        if not need_state:
            return None
        ns = ops.default_noise(self.edges.device)
        ns.advance()
        return ns.state

    def sample(self, n: int, u: Optional[torch.Tensor] = None, v: Optional[torch.Tensor] = None):
        """sample_distribution (main_vae.py:427-436) for mu and logvar: -> (mu, logvar), f32 [n, L] each (views of one
        [n, 2L] tensor).  u, v: f64 [n, 2L] on the device inject the two uniforms of every element (u picks the bin, v the
        place inside it); by default they come from the device stream, which advances by one step per call."""
        state = self._draws(u, v, u is None)
        mulv, _ = ops.latent_sample(self.edges, self.cdf, self.latent_dim, n, u, v, None, state)
        return mulv[:, :self.latent_dim], mulv[:, self.latent_dim:]

    def sample_z(self, n: int, dtype_of=None, u=None, v=None, eps=None, return_mulv: bool = False):
        """``z = mu + exp(0.5 * logvar) * randn`` (main_vae.py:482-488) of n draws in ONE launch, in the input layout of
        the decoder ``dtype_of`` ([n, 1, 1, ZP] in its engine dtype, pad columns zero; f32 when dtype_of is None).
        eps: f32 [n, L] injects the normal draw.  The engine's reparameterisation clamps logvar to [-10, 10]
        (vaegan_code.py:75; :487 does not -- inert for |logvar| < 10).  return_mulv: -> (z, mulv f32 [n, 2L])."""
        L = self.latent_dim
        dt = G.F32 if dtype_of is None else dtype_of._dt
        nz = L if dtype_of is None else dtype_of.nz
        if nz != L:
            raise RuntimeError(f"LatentPrior.sample_z: the decoder takes nz = {nz} inputs, the prior has {L} dimensions")
        state = self._draws(u, v, u is None or eps is None)
        mulv, z = ops.latent_sample(self.edges, self.cdf, L, n, u, v, eps, state, want_mulv=return_mulv,
                                    z=(G.padc(nz, dt), dt))
        return (z, mulv) if return_mulv else z

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """Plain tensors: save a fitted prior beside the decoder checkpoint and sample without the data set."""
        return {"edges": self.edges, "counts": self.counts, "cdf": self.cdf,
                "latent_dim": torch.tensor(self.latent_dim), "n_fitted": torch.tensor(self.n_fitted)}

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> "LatentPrior":
        """Replace this prior's tables by those of ``sd`` (a ``state_dict()``, e.g. from torch.load), moved to its device."""
        dev = self.edges.device
        self.__init__(sd["edges"].to(dev), sd["counts"].to(dev), sd["cdf"].to(dev), int(sd["latent_dim"]),
                      int(sd["n_fitted"]))
        return self

    @classmethod
    def from_state_dict(cls, sd: Dict[str, torch.Tensor], device="cuda") -> "LatentPrior":
        return cls(sd["edges"].to(device), sd["counts"].to(device), sd["cdf"].to(device), int(sd["latent_dim"]),
                   int(sd["n_fitted"]))


def _device_of(decoder, what: str):
    dev = next(decoder.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError(f"{what} needs the decoder on the MI355X ('cuda'); there is no CPU path")
    return dev


def _decode(decoder, z_nhwc: torch.Tensor, b: int) -> torch.Tensor:
    """Generator forward from its engine input -> tanh image NCHW f32; the launches of Generator.forward."""
    if decoder.fused_tail(b):
        img, _ = decoder.engine_forward(z_nhwc, b, keep=False, tail={})
        return img
    pre, _ = decoder.engine_forward(z_nhwc, b, keep=False)
    return ops.nhwc_to_nchw(pre, decoder.nc, decoder._dt, apply_tanh=True)


def _normal_z(decoder, b: int, eps: Optional[torch.Tensor]) -> torch.Tensor:
    """z ~ N(0, I) [b, nz] (main_vae.py:552-553, :364-365) in the decoder's input layout."""
    dt = decoder._dt
    dev = next(decoder.parameters()).device
    if eps is None:
        ns = ops.default_noise(dev)
        ns.advance()
        eps = ns.randn((b, decoder.nz), ops.DRAW_LATENT_EPS)
    if not eps.is_cuda:
        raise RuntimeError("generation needs the latent draws on the MI355X ('cuda'); there is no CPU path")
    if eps.dtype != torch.float32 or eps.numel() != b * decoder.nz:
        raise RuntimeError(f"z must be f32 [{b}, {decoder.nz}(, 1, 1)]")
    return ops.nchw_to_nhwc(eps.contiguous().view(b, decoder.nz, 1, 1), G.padc(decoder.nz, dt), dt)


@torch.no_grad()
def evaluate_generation(decoder, val_loader: Iterable[torch.Tensor], prior: Optional[LatentPrior] = None,
                        noise_fn=None, feature_fn=None, k: int = 3, real_stats=None, kid_subsets: Optional[int] = None,
                        kid_subset_size: int = 1000, kid_seed: int = 0) -> Dict[str, float]:
    """The generation-evaluation loops of the reference:

        decoder.eval()                                                                  (main_vae.py:476 / :546)
        for real in val_loader:   b = real.size(0)
            prior given  (:482-489): mu, logvar ~ histogram prior; z = mu + exp(logvar / 2) * randn; fake = G(z)
            prior=None   (:552-554): z = randn(b, latent); fake = G(z)
            ssim.update((fake + 1) / 2, (real + 1) / 2)                                 (:492-496 / :557-561)
        ssim.compute()                                                   (mean over all images, ragged batch weighted)

    val_loader yields device batches [b,C,S,S] in [-1,1] (data.DeviceLoader).  noise_fn(i, b) injects the draws of batch
    i (parity tests): with a prior it returns (u, v, eps) -- f64 [b,2L], f64 [b,2L], f32 [b,L], see LatentPrior.sample_z --
    and without one the f32 [b, nz] z itself; by default everything is drawn on the device.  SSIM: torchmetrics recipe,
    parity unpinned (the package is not installed), as in denoise.py.  Deviation: the logvar clamp of sample_z.
    Accumulation stays on the device; ONE host sync at the end of the pass.  Returns python numbers: ssim, samples,
    batches.

    feature_fn (default None: nothing below happens and exactly the three keys above come back): a callable
    ``images_u8 [b,C,S,S] uint8 device -> f32 [b, D] device`` -- ``metrics.encoder_features(encoder)`` or a network of
    the caller's (the reference's InceptionV3, :472-473).  Each batch's real and fake images go through ``ops.to_u8``
    (:492, :498-499) and feature_fn; ``fid.update`` (:500-501) becomes two f64 running-sum kernels per batch, the
    features stay on the device for the pass, and the result gains ``fid`` (:507), ``precision``, ``recall``, ``f1``
    (README.md:22, k-th-neighbour manifolds with ``k``) and ``feature_dim``.  real_stats: a ``metrics.FeatureStats`` of the
    real side computed earlier (the reference recomputes it on every call): the real half of the FID update is skipped.
    Inception Score needs InceptionV3's classifier head: out of scope.  Still one host sync for everything accumulated on
    the device, plus the final D x D step of ``metrics.frechet_distance`` on the host.

    kid_subsets (default None: nothing changes; needs feature_fn, else RuntimeError): the Kernel Inception Distance of the
    pass's features (``metrics.kernel_distance``: ``kid_subsets`` subset pairs of ``kid_subset_size`` rows drawn on the host
    with ``kid_seed``, degree 3, gamma 1 / D, coef 1); the result gains ``kid_mean`` and ``kid_std`` (population standard
    deviation), read in the same host sync.  Not in the reference; single process, like precision / recall."""
    if kid_subsets is not None and feature_fn is None:
        raise RuntimeError("evaluate_generation: kid_subsets needs a feature_fn (KID is a feature-space metric)")
    decoder.eval()
    dev = _device_of(decoder, "evaluate_generation")
    acc = ops.zeros_f32(1, dev)
    seen = batches = 0
    feats = FeaturePass(feature_fn, True, real_stats) if feature_fn is not None else None
    for i, real in enumerate(val_loader):
        if not real.is_cuda:
            raise RuntimeError("evaluate_generation needs device batches (data.DeviceLoader); there is no CPU path")
        real = real.contiguous()
        b = real.shape[0]
        inj = noise_fn(i, b) if noise_fn is not None else None
        if prior is not None:
            u, v, eps = inj if inj is not None else (None, None, None)
            z = prior.sample_z(b, decoder, u, v, eps)
        else:
            z = _normal_z(decoder, b, inj)
        fake = _decode(decoder, z, b)
        ops.axpy(acc, ops.ssim(fake, real), float(b), out=acc)
        if feats is not None:
            feats.update(real, fake)
        seen += b
        batches += 1
    if batches == 0:
        raise RuntimeError("evaluate_generation: the loader yielded no batch")
    if feats is None:
        return {"ssim": float(acc.item()) / seen, "samples": seen, "batches": batches}   # the one host sync
    counts = feats.pr_counts(int(k))
    parts = [acc.double(), counts.double()]
    if kid_subsets is not None:
        parts.append(feats.kid(int(kid_subsets), int(kid_subset_size), int(kid_seed)))
    ssim_sum, fake_in_real, real_in_fake, *kid = torch.cat(parts).tolist()             # the one host sync
    out = {"ssim": ssim_sum / seen, "samples": seen, "batches": batches, "fid": feats.fid(), "feature_dim": feats.D}
    pr = _pr_result(int(fake_in_real), int(real_in_fake), seen, seen, int(k))
    out.update(precision=pr["precision"], recall=pr["recall"], f1=pr["f1"])
    if kid:
        out.update(kid_mean=kid[0], kid_std=kid[1])
    return out


@torch.no_grad()
def sample_images(decoder, z: Optional[torch.Tensor] = None, n: int = 64, prior: Optional[LatentPrior] = None,
                  grid_cols: int = 0) -> torch.Tensor:
    """Generated images as uint8 on the device ((fake + 1) / 2 * 255, clamped and truncated: main_vae.py:492,498-499), the
    decoder in eval mode:
        z=None, prior=None: n images from z ~ N(0, I)                        (sample_vae_decoder, main_vae.py:364-366)
        z f32 [n, nz, 1, 1]: the images of that z -- the per-epoch ``decoder(fixed_noise)`` picture, vaegan_code.py:40, 209-216
        prior:              n images from the histogram prior                (sample_vae, main_vae.py:619-626)
    grid_cols == 0: [n, C, S, S]; grid_cols > 0: ONE [rows*S, grid_cols*S, C] picture, image i at tile (i // grid_cols,
    i % grid_cols), ready for ``PIL.Image.fromarray(out.cpu().numpy())``."""
    decoder.eval()
    _device_of(decoder, "sample_images")
    if z is not None:
        if prior is not None:
            raise RuntimeError("sample_images: give z or a prior, not both")
        if z.dim() != 4 or z.shape[1] != decoder.nz or z.shape[2] != 1 or z.shape[3] != 1:
            raise RuntimeError(f"sample_images: z must be [n, {decoder.nz}, 1, 1], got {tuple(z.shape)}")
        n = z.shape[0]
        zh = _normal_z(decoder, n, z)
    elif prior is not None:
        zh = prior.sample_z(n, decoder)
    else:
        zh = _normal_z(decoder, n, None)
    return ops.to_u8(_decode(decoder, zh, n), grid_cols)
