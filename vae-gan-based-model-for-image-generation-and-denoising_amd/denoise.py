"""Denoising evaluation path of the reference (vaegan_code.py:147-171; BASELINE config 4): eval-mode Encoder ->
reparameterisation -> Generator on ``clamp(img + sigma*eps, -1, 1)``, reconstruction MSE + KL (not divided by
the batch, :166), and image-quality metrics on the [0,1]-rescaled images: SSIM (torchmetrics recipe, parity
unpinned: the package is not installed) and PSNR (listed as intended in the reference README.md:22, implemented
nowhere in it).  All compute is HIP kernels.  FID (vaegan_code.py:182-183) is computed in the feature space of a pluggable
``feature_fn`` (metrics.py); InceptionV3 itself needs downloaded weights, so Inception Score is out of scope.
"""
import math
from typing import Dict, Iterable, Optional

import torch

from . import geometry as G
from . import ops
from . import tiling
from .baselines import NLMeans, check_oracle_sigma, make_baseline
from .capture import HostMirrors, capture, replay
from .engine import GradSink
from .metrics import FeaturePass


def _default_draws(dev, eps_shape, z_shape):
    """The default draws of one batch: ONE advance() of the device noise stream (HIP Philox, keyed by torch's device seed),
    then draw 0 = the image noise and draw 1 = the latent noise.  A shape of None: that draw is not generated.
    -> (eps or None, eps_z or None)"""
    ns = ops.default_noise(dev)
    ns.advance()
    return (None if eps_shape is None else ns.randn(tuple(eps_shape), 0),
            None if z_shape is None else ns.randn(tuple(z_shape), 1))


def _reconstruct(encoder, decoder, noisy_h, b: int, eps_z, train_e: bool = False, train_g: bool = False, out=None):
    """The reconstruction step of every pass (vaegan_code.py:158-163, main_vae.py:258-260): Encoder on the NHWC input ->
    reparameterise with eps_z -> Generator -> Tanh into an NCHW f32 image (``out``: written there).
    -> (recon, mulv [b, MP], the clamped logvar)"""
    dt = encoder._dt
    mulv, _ = encoder._engine.forward(noisy_h, b, train_e, keep=False)
    mulv = mulv.view(b, -1)
    z, lvc = ops.reparam_forward(mulv, eps_z, encoder.latent_dim, G.padc(decoder.nz, dt), dt)
    pre, _ = decoder._engine.forward(z, b, train_g, keep=False)
    return ops.nhwc_to_nchw(pre, decoder.nc, dt, apply_tanh=True, out=out), mulv, lvc


def _psnr(mse: float) -> float:
    mse01 = mse / 4.0                                                      # ((a+1)/2 - (b+1)/2)^2 = (a-b)^2 / 4
    return float("inf") if mse01 == 0 else 10.0 * math.log10(1.0 / mse01)


def _region_keys(suffix: str, sums) -> Dict[str, float]:
    """{S_hole, S_valid, n_hole, n_valid} of a pass -> the five region keys; an empty region reports mse 0.0 and psnr inf."""
    s_hole, s_valid, n_hole, n_valid = sums
    m_hole = s_hole / n_hole if n_hole > 0 else 0.0
    m_valid = s_valid / n_valid if n_valid > 0 else 0.0
    return {"mse_hole" + suffix: m_hole, "mse_valid" + suffix: m_valid, "psnr_hole" + suffix: _psnr(m_hole),
            "psnr_valid" + suffix: _psnr(m_valid), "hole_fraction" + suffix: n_hole / (n_hole + n_valid)}


class _Quality:
    """What every pass measures of ONE candidate image (the reconstruction, the noisy input, the refined reconstruction, the
    filtered image) against the clean one: per batch the MSE and the mean SSIM, with ms_ssim the MS-SSIM, each added times the
    batch's image count into its own f32 slot on the device, and with regions the f64 {S_hole, S_valid, n_hole, n_valid} that
    ops.region_mse_forward_backward accumulates.  ``_allocate`` gives the candidates of a pass their slots, ``_read`` is the
    pass's one host read, and ``result`` names this candidate's part of it with its suffix.  A further candidate is one more
    instance."""

    def __init__(self, suffix: str, ms_ssim: bool = False, regions: bool = False):
        self.suffix, self.ms_ssim, self.regions = suffix, ms_ssim, regions
        self.slots = 3 if ms_ssim else 2                # f32: [sum(b * mse), sum(b * ssim)(, sum(b * ms_ssim))]
        self.acc = self.stats = None                    # _allocate: one view per slot, the f64 [4] region statistics

    def update(self, x, clean, b: int, rects=None, mse=None, store: bool = False) -> None:
        """mse: the f32 slot holding mse_mean(x, clean) when the pass has computed it already.  store=True (a pass of one
        batch, weight 1): the MSE kernel writes its slot itself, no add."""
        if store:
            ops.mse_forward_backward(x, clean, 1.0, self.acc[0], False)
        else:
            if mse is None:
                mse = torch.empty(1, dtype=torch.float32, device=clean.device)
                ops.mse_forward_backward(x, clean, 1.0, mse, False)
            ops.axpy(self.acc[0], mse, float(b), out=self.acc[0])
        ops.axpy(self.acc[1], ops.ssim(x, clean), float(b), out=self.acc[1])
        if self.ms_ssim:
            ops.axpy(self.acc[2], ops.ms_ssim(x, clean), float(b), out=self.acc[2])
        if self.regions:
            ops.region_mse_forward_backward(x, clean, rects, 1.0, 1.0, stats=self.stats)   # w_hole = 1, no gradient

    def result(self, sums, stats, seen: int):
        """Host only.  sums: this candidate's f32 slots as read, stats: its four region sums (None without regions)
        -> (its recon_loss / ssim / psnr keys, its ms_ssim key or {}, its five region keys or {}), all carrying the suffix."""
        s = self.suffix
        mse_sum, ssim_sum, *ms_sum = sums
        main = {"recon_loss" + s: mse_sum / seen, "ssim" + s: ssim_sum / seen, "psnr" + s: _psnr(mse_sum / seen)}
        ms = {"ms_ssim" + s: ms_sum[0] / seen} if self.ms_ssim else {}
        return main, ms, _region_keys(s, stats) if self.regions else {}


def _allocate(dev, own: int, qs) -> torch.Tensor:
    """The device sums of a pass in ONE zeroed f32 buffer: ``own`` slots of the pass itself, then the slots of every candidate
    in qs, front to back; a candidate with regions gets its f64 statistics beside it.  -> the buffer"""
    buf = ops.zeros_f32(own + sum(q.slots for q in qs), dev)
    at = own
    for q in qs:
        q.acc, at = [buf[i:i + 1] for i in range(at, at + q.slots)], at + q.slots
        q.stats = torch.zeros(4, dtype=torch.float64, device=dev) if q.regions else None
    return buf


def _read(buf, qs) -> list:
    """The ONE host sync of a pass -> _allocate's buffer, then the region statistics of every candidate that has them (the
    f32 slots are widened to sit next to them, which is exact)."""
    stats = [q.stats for q in qs if q.regions]
    return (torch.cat([buf.double()] + stats) if stats else buf).tolist()


def _results(qs, host, own: int, seen: int) -> list:
    """Cut _read's list as _allocate laid it out, front to back -> the ``result`` of every candidate."""
    out, at, st = [], own, own + sum(q.slots for q in qs)
    for q in qs:
        out.append(q.result(host[at:at + q.slots], host[st:st + 4] if q.regions else None, seen))
        at, st = at + q.slots, st + (4 if q.regions else 0)
    return out


def _add_optional(out: dict, base, further=()) -> dict:
    """The keys behind the flags, in the passes' order: the ms_ssim key of every ``base`` candidate (the reconstruction, the
    noisy input), then their region keys; a ``further`` candidate (refined, nlm) reports all it has, together."""
    for kind in (1, 2):
        for r in base:
            out.update(r[kind])
    for cand in further:
        for part in cand:
            out.update(part)
    return out


@torch.no_grad()
def denoise_eval(encoder, decoder, img: torch.Tensor, sigma: float = 0.05, eps: Optional[torch.Tensor] = None,
                 eps_z: Optional[torch.Tensor] = None, alpha_kl: float = 0.1,
                 noisy: Optional[torch.Tensor] = None, ms_ssim: bool = False) -> Dict[str, object]:
    """img: [B,C,S,S] float32 on the MI355X in [-1,1].  Returns the noisy input, the reconstruction (both NCHW
    f32) and a dict of device scalars + host floats: recon_loss, kl_loss (sum), val_loss, psnr, ssim.
    ms_ssim=True (default False: exactly the keys and the launches above) adds ``ms_ssim``, the multi-scale SSIM of the
    reconstruction (ops.ms_ssim with the default scales of the image size), read in the host sync that reads ssim.
    noisy: an already degraded input batch (the ``noisy`` half of a data.DeviceLoader pair) used INSTEAD of
    clamp(img + sigma*eps): sigma / eps are then ignored, img is the clean target.
    The caller puts encoder / decoder in eval mode (vaegan_code.py:147-148) -- or not: BatchNorm follows
    module.training exactly as in the reference."""
    if not img.is_cuda:
        raise RuntimeError("denoise_eval needs the batch on the MI355X ('cuda'); there is no CPU path")
    dt = encoder._dt
    B, C = img.shape[0], img.shape[1]
    img = img.contiguous()
    draw_eps = eps is None and noisy is None
    if draw_eps or eps_z is None:
        drawn = _default_draws(img.device, img.shape if draw_eps else None, (B, encoder.latent_dim) if eps_z is None else None)
        eps, eps_z = drawn[0] if draw_eps else eps, drawn[1] if eps_z is None else eps_z
    if noisy is not None:
        if not noisy.is_cuda or noisy.shape != img.shape:
            raise RuntimeError("denoise_eval: noisy must be a device batch of img's shape")
        noisy = noisy.contiguous()
        noisy_h = ops.nchw_to_nhwc(noisy, G.padc(C, dt), dt)
    else:
        noisy_h, noisy = ops.noisy_clamp_to_nhwc(img, eps, sigma, G.padc(C, dt), dt)
    recon, mulv, lvc = _reconstruct(encoder, decoder, noisy_h, B, eps_z, encoder.training, decoder.training)
    scal = ops.zeros_f32(4, img.device)
    ops.mse_forward_backward(recon, img, 1.0, scal[0:1], False)            # recon_loss (:165)
    ops.kl_forward(mulv, lvc, encoder.latent_dim, 1.0, dt, out=scal[1:2])  # KL sum, no /B (:166)
    ssim_t = ops.ssim(recon, img)
    recon_loss, kl = (float(v) for v in scal[:2].tolist())
    out = {"noisy": noisy, "recon": recon, "recon_loss": recon_loss, "kl_loss": kl,
           "val_loss": recon_loss + alpha_kl * kl, "psnr": _psnr(recon_loss)}
    if ms_ssim:
        out["ssim"], out["ms_ssim"] = torch.cat([ssim_t, ops.ms_ssim(recon, img)]).tolist()
    else:
        out["ssim"] = float(ssim_t.item())
    return out


@torch.no_grad()
def validation_epoch(encoder, decoder, loader: Iterable[torch.Tensor], n_samples: Optional[int] = None,
                     sigma: float = 0.05, alpha_kl: float = 0.1, noise_fn=None, feature_fn=None,
                     kid_subsets: Optional[int] = None, kid_subset_size: int = 1000, kid_seed: int = 0,
                     ms_ssim: bool = False) -> Dict[str, float]:
    """The per-epoch validation loop of the reference trainer, vaegan_code.py:147-191:

        encoder.eval(); decoder.eval()                                   (:147-148; the discriminator is not used)
        for img in val_loader:   noisy = clamp(img + 0.05*randn, -1, 1) -> E -> reparameterise -> G
            val_loss += mse_mean(recon, img) + alpha_kl * KL_sum          (:165-167: ONE number per batch)
            ssim.update((recon+1)/2, (img+1)/2)                           (:170-174)
        val_loss /= len(val_loader.dataset)                               (:187: divided by the SAMPLE count)
        ssim.compute()                                                    (:185: mean over all validation images)

    loader yields device batches [b,C,S,S] in [-1,1] (data.DeviceLoader; the ragged last batch counts with its own
    size, as torchmetrics' running sums do).  n_samples defaults to the number of images seen (= len(dataset) for a
    full pass).  noise_fn(i, img) -> (eps, eps_z) injects the two draws of batch i (parity tests); by default they are
    generated on the device.  PSNR (not in the reference, README.md:22 lists it as intended) is that of the mean
    squared error over every pixel of the pass.  Accumulation stays on the device; ONE host sync at the end of the pass.
    Returns python floats: val_loss, ssim, psnr, recon_loss (mean of the batch MSEs), kl_loss (mean of the batch KL
    sums), samples, batches.
    feature_fn (default None: nothing changes): ``images_u8 [b,C,S,S] uint8 device -> f32 [b, D] device``
    (``metrics.encoder_features(encoder)`` or a network of the caller's): the reconstructions and the clean images go
    through ``ops.to_u8`` and feature_fn, their f64 running statistics are accumulated on the device per batch
    (fid.update, :182-183) and the result gains ``fid`` (fid.compute, :185; its last D x D step runs on the host, see
    ``metrics.frechet_distance``).  Inception Score needs InceptionV3's classifier head: out of scope.
    kid_subsets (default None: nothing changes; needs feature_fn, else RuntimeError): the pass keeps its features on the
    device and the result gains ``kid_mean`` and ``kid_std``, the Kernel Inception Distance between the clean images and
    the reconstructions (``metrics.kernel_distance``: ``kid_subsets`` subset pairs of ``kid_subset_size`` rows drawn on the
    host with ``kid_seed``; population standard deviation).  Not in the reference; single process; one more host read of
    two doubles.
    ms_ssim=True (default False: nothing changes): the result gains ``ms_ssim``, the multi-scale SSIM (ops.ms_ssim, the
    default scales of the image size) accumulated like ssim -- the batch's value times its image count, on the device -- and
    read in the same host sync."""
    if kid_subsets is not None and feature_fn is None:
        raise RuntimeError("validation_epoch: kid_subsets needs a feature_fn (KID is a feature-space metric)")
    encoder.eval(), decoder.eval()                                                   # :147-148
    dev = next(encoder.parameters()).device
    qs = [_Quality("", ms_ssim)]                                                     # :170-174 (ssim.update), MSE for the PSNR
    sums = _allocate(dev, 2, qs)                                                     # [sum(recon + a*kl), sum(kl)], the candidate's
    seen = batches = 0
    dt, L = encoder._dt, encoder.latent_dim
    feats = FeaturePass(feature_fn, kid_subsets is not None) if feature_fn is not None else None
    for i, img in enumerate(loader):
        if not img.is_cuda:
            raise RuntimeError("validation_epoch needs device batches (data.DeviceLoader); there is no CPU path")
        img = img.contiguous()
        b, C = img.shape[0], img.shape[1]
        eps, eps_z = noise_fn(i, img) if noise_fn is not None else _default_draws(dev, img.shape, (b, L))
        noisy_h, _ = ops.noisy_clamp_to_nhwc(img, eps, sigma, G.padc(C, dt), dt)     # :153-154
        recon, mulv, lvc = _reconstruct(encoder, decoder, noisy_h, b, eps_z)         # :160-163
        scal = torch.empty(2, dtype=torch.float32, device=dev)
        ops.mse_forward_backward(recon, img, 1.0, scal[0:1], False)                  # :165
        ops.kl_forward(mulv, lvc, L, 1.0, dt, out=scal[1:2])                         # :166 (sum, not / B)
        ops.axpy(sums[0:1], scal[0:1], 1.0, out=sums[0:1])
        ops.axpy(sums[0:1], scal[1:2], alpha_kl, out=sums[0:1])                      # :167
        ops.axpy(sums[1:2], scal[1:2], 1.0, out=sums[1:2])
        qs[0].update(recon, img, b, mse=scal[0:1])
        if feats is not None:
            feats.update(img, recon)
        seen += b
        batches += 1
    if batches == 0:
        raise RuntimeError("validation_epoch: the loader yielded no batch")
    kid = feats.kid(int(kid_subsets), int(kid_subset_size), int(kid_seed)) if kid_subsets is not None else None
    out = _validation_result(qs, _read(sums, qs), seen, batches, seen if n_samples is None else int(n_samples))
    if feats is not None:
        out["fid"] = feats.fid()
    if kid is not None:
        out["kid_mean"], out["kid_std"] = kid.tolist()
    return out


@torch.no_grad()
def paired_test_epoch(encoder, decoder, loader: Iterable, n_samples: Optional[int] = None, noise_fn=None,
                      regions: bool = False, ms_ssim: bool = False, refine=None, baseline=None) -> Dict[str, float]:
    """The reference's test pass over (noisy, clean) pairs, main_vae.py:251-266:

        encoder.eval(); decoder.eval()                                                 (:251-252)
        for noisy, clean in test_loader:   mu, logvar = E(noisy); z = mu + exp(logvar/2) * randn; recon = G(z)
            test_loss += mse_SUM(recon, clean) + KL_sum                                 (:262-264)
        test_loss /= len(test_loader.dataset)                                          (:266)

    and, beyond the reference, SSIM and PSNR (on the [0,1]-rescaled images, as validation_epoch) of ``recon`` vs ``clean``
    AND of ``noisy`` vs ``clean``, so the caller sees what the model gained over its input.  The metrics assume images
    in [-1, 1] (``Degrade(normalize=True)``).
    loader yields device pairs (data.DeviceLoader with a ``Degrade``).  A loader that offers ``want_nhwc`` is asked to
    write ``noisy`` in the Encoder's input layout in the same kernel pass (no separate layout pass per batch).
    noise_fn(i, noisy) -> eps_z [b, L] injects the reparameterisation draw of batch i (parity tests); by default it is
    generated on the device.  n_samples defaults to the number of images seen.
    Deviation: the engine's reparameterisation clamps logvar to [-10, 10] (as the training path, vaegan_code.py:76);
    :258-259 do not.  Inert for |logvar| < 10.
    Accumulation stays on the device; ONE host sync at the end.  Returns python floats: test_loss, recon_loss (mean
    squared error per element), kl_loss (mean KL sum per sample), ssim, psnr, ssim_noisy, psnr_noisy, samples, batches.
    regions=True (default False: exactly the keys and the launches above): the loader must offer ``want_rects`` (a degraded
    data.DeviceLoader); the pass turns it on and restores it.  The result gains mse_hole, mse_valid (mean squared error per
    element inside / outside the occlusion rectangles), psnr_hole, psnr_valid and hole_fraction (hole elements / all
    elements) of ``recon`` vs ``clean``, and the same five suffixed ``_noisy`` for the input, each set from one f64[4]
    tensor that ops.region_mse_forward_backward accumulates over the pass (w_hole = 1, no gradient).  An empty region
    reports mse 0.0 and psnr inf.  Still one host sync.
    ms_ssim=True (default False: nothing changes): the result gains ``ms_ssim`` and ``ms_ssim_noisy``, the multi-scale SSIM
    (ops.ms_ssim, the default scales of the image size) of ``recon`` and of ``noisy`` vs ``clean``, accumulated like ssim and
    read in the same host sync.
    refine (default None: exactly the keys and the launches above): a ``LatentRefiner`` built on these networks, or a dict of
    its keywords (``discriminator=`` among them) from which one is built.  Every batch is ALSO refined at test time --
    ``refine.refine(noisy, rects=loader.last_rects)`` from the Encoder's mean, the occlusion rectangle left out of its loss
    -- and the result gains ``recon_loss_refined``, ``ssim_refined`` and ``psnr_refined`` of the refined reconstruction vs
    ``clean`` (with regions=True also the five region keys suffixed ``_refined``), accumulated on the device and read in the
    same host sync.  The loader must offer ``want_rects``, which the pass turns on and restores as regions=True does.
    baseline (default None: exactly the keys and the launches above): a ``baselines.NLMeans``, the string "nlm" (its
    defaults) or a dict of its keywords.  Every noisy batch ALSO goes through non-local means -- the classical, parameter-free
    denoiser between the input and the model -- and the result gains ``recon_loss_nlm``, ``ssim_nlm`` and ``psnr_nlm`` of its
    output vs ``clean`` (with ms_ssim=True also ``ms_ssim_nlm``, with regions=True also the five region keys suffixed
    ``_nlm``), accumulated on the device and read in the same host sync.  ``sigma="oracle"`` (NLMeans' default) reads the
    noise level the loader drew per image, ``loader.last_rects[:, 1]``, in place: it needs a degraded loader, whose
    ``want_rects`` the pass turns on and restores; ``"estimate"`` (blind, ops.noise_sigma) and a number need no rectangles.
    That level is a Gaussian sigma only under the default ``Degrade``: with another noise_model or with impulses "oracle" raises
    ValueError.  A ``baselines.Median``, "median" or ``{"radius": r}`` runs the median filter instead -- the baseline that means
    something under impulse noise -- and the same keys come suffixed ``_median``."""
    nlm = make_baseline("paired_test_epoch", baseline)
    check_oracle_sigma("paired_test_epoch", nlm, loader)
    refiner = None
    if refine is not None:
        if isinstance(refine, LatentRefiner):
            refiner = refine
        elif isinstance(refine, dict):
            refiner = LatentRefiner(encoder, decoder, **refine)
        else:
            raise ValueError("paired_test_epoch: refine must be a LatentRefiner or a dict of its keywords")
        if refiner.E is not encoder or refiner.G is not decoder:
            raise ValueError("paired_test_epoch: the LatentRefiner was built on other networks")
    need_rects = regions or refiner is not None or (nlm is not None and nlm.needs_rects)
    if need_rects and not (hasattr(loader, "want_rects") and getattr(loader, "degrade", None) is not None and loader.degrade.pairs):
        why = "regions=True" if regions else ("refine" if refiner is not None else "baseline with sigma='oracle'")
        raise RuntimeError(f"paired_test_epoch: {why} needs a degraded data.DeviceLoader "
                           f"(want_rects)")
    encoder.eval(), decoder.eval()                                                   # :251-252
    dev = next(encoder.parameters()).device
    dt, L = encoder._dt, encoder.latent_dim
    recon_q, noisy_q = _Quality("", ms_ssim, regions), _Quality("_noisy", ms_ssim, regions)
    refined_q = _Quality("_refined", False, regions) if refiner is not None else None
    nlm_q = _Quality("_" + nlm.name, ms_ssim, regions) if nlm is not None else None
    qs = [q for q in (recon_q, noisy_q, refined_q, nlm_q) if q is not None]
    sums = _allocate(dev, 2, qs)                                                     # [sum(mse_sum + kl), sum(kl)], the candidates'
    seen = batches = 0
    offers = hasattr(loader, "want_nhwc") and getattr(loader, "degrade", None) is not None and loader.degrade.pairs
    if offers:
        loader.want_nhwc(G.padc(loader.dataset.image_shape[0], dt), dt)
    if need_rects:
        rects_were_on = bool(getattr(loader, "_rects", False))
        loader.want_rects(True)
    try:
        for i, (noisy, clean) in enumerate(loader):
            if not (noisy.is_cuda and clean.is_cuda):
                raise RuntimeError("paired_test_epoch needs device pairs (data.DeviceLoader); there is no CPU path")
            noisy, clean = noisy.contiguous(), clean.contiguous()
            b, C = clean.shape[0], clean.shape[1]
            noisy_h = loader.last_nhwc if offers else ops.nchw_to_nhwc(noisy, G.padc(C, dt), dt)
            rects = loader.last_rects if need_rects else None
            eps_z = noise_fn(i, noisy) if noise_fn is not None else None
            if eps_z is None:
                eps_z = _default_draws(dev, None, (b, L))[1]
            recon, mulv, lvc = _reconstruct(encoder, decoder, noisy_h, b, eps_z)     # :258-260
            scal = torch.empty(2, dtype=torch.float32, device=dev)
            ops.mse_forward_backward(recon, clean, 1.0, scal[0:1], False)            # mean; * numel = :262's sum
            ops.kl_forward(mulv, lvc, L, 1.0, dt, out=scal[1:2])                     # :263
            ops.axpy(sums[0:1], scal[0:1], float(clean.numel()), out=sums[0:1])
            ops.axpy(sums[0:1], scal[1:2], 1.0, out=sums[0:1])                       # :264
            ops.axpy(sums[1:2], scal[1:2], 1.0, out=sums[1:2])
            recon_q.update(recon, clean, b, rects, mse=scal[0:1])
            noisy_q.update(noisy, clean, b, rects)
            if refiner is not None:
                refined_q.update(refiner.refine(noisy, rects=rects)["recon"], clean, b, rects)
            if nlm is not None:
                nlm_q.update(nlm(noisy, rects=rects if nlm.needs_rects else None), clean, b, rects)
            seen += b
            batches += 1
    finally:
        if offers:
            loader.want_nhwc(None)
        if need_rects:
            loader.want_rects(rects_were_on)
    if batches == 0:
        raise RuntimeError("paired_test_epoch: the loader yielded no batch")
    return _paired_result(qs, _read(sums, qs), seen, batches, seen if n_samples is None else int(n_samples))


def _validation_result(qs, host, seen: int, batches: int, n: int) -> Dict[str, float]:
    """Host only.  host: validation_epoch's read, [sum(recon + a*kl), sum(kl)] then the reconstruction's slots."""
    (r,) = _results(qs, host, 2, seen)
    out = {"val_loss": host[0] / n, "ssim": r[0]["ssim"], "psnr": r[0]["psnr"], "recon_loss": r[0]["recon_loss"],
           "kl_loss": host[1] / batches, "samples": seen, "batches": batches}
    return _add_optional(out, (r,))


def _paired_result(qs, host, seen: int, batches: int, n: int) -> Dict[str, float]:
    """Host only.  host: paired_test_epoch's read, [sum(mse_sum + kl), sum(kl)] then the sums of every candidate in qs: the
    reconstruction, the noisy input and whichever further candidates (refined, nlm) the pass had."""
    r, noisy, *further = _results(qs, host, 2, seen)
    out = {"test_loss": host[0] / n, "recon_loss": r[0]["recon_loss"], "kl_loss": host[1] / seen, "ssim": r[0]["ssim"],
           "psnr": r[0]["psnr"], "ssim_noisy": noisy[0]["ssim_noisy"], "psnr_noisy": noisy[0]["psnr_noisy"],
           "samples": seen, "batches": batches}
    return _add_optional(out, (r, noisy), further)


def _finite_nonneg(name: str, v) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not (math.isfinite(v) and v >= 0.0):
        raise ValueError(f"{name} must be finite and >= 0")
    return float(v)


class LatentRefiner:
    """Test-time latent refinement (not in the reference; GAN-inversion denoising / inpainting, Yeh et al. 2017, "Semantic
    image inpainting with deep generative models"): keep the trained networks frozen, start from the Encoder's latent and
    run Adam on z so that G(z) matches the degraded input OUTSIDE its occlusion rectangle, optionally with the Discriminator
    as a realism prior and a Gaussian prior on z.  Per image i the objective is

        J_i = mse_valid_i(G(z_i), noisy_i) + alpha_adv * (-max(log D(G(z_i)), -100)) + prior_weight * |z_i|^2 / (2 L)

    (mse_valid_i: mean squared error over the elements outside image i's rectangle).  The adversarial term DESCENDS along the
    gradient of BCE(D(G(z)), 0.9) -- the trainer's smoothed "real" label -- while J reports the unsmoothed -log D.
    All arithmetic is eval-mode (BatchNorm on the running statistics, whatever ``module.training`` says; the flags are left
    alone): rows are independent, no parameter, buffer, ``num_batches_tracked`` or ``.grad`` is touched, no weight gradient
    is formed.  One iteration = G forward (kept), ops.masked_mse_rows, [D forward, head launch, D data gradients,
    ops.nchw_grad_add_to_nhwc |  ops.nchw_grad_to_nhwc], G data gradients, ops.latent_adam -- DESIGN.md section 4.4q.
    graphed=True replays ONE captured iteration ``steps`` times (capture.capture / capture.replay); a capture is keyed by the
    batch size and by what the engines key their packed operands by, so a refiner used between training steps captures
    again.  encoder=None builds a refiner that only takes an injected start (``init=`` a tensor; the Encoder needs images of
    at least 64 x 64, the other two networks go down to 16 x 16).  keep_best=True returns, per image, the iterate with the lowest objective seen (the start included)."""

    REAL_LABEL = 0.9                        # VAEGANTrainer's real_label default (vaegan_code.py:88)

    def __init__(self, encoder, decoder, discriminator=None, *, steps: int = 50, lr: float = 0.05, betas=(0.9, 0.999),
                 eps: float = 1e-8, alpha_adv: float = 0.0, prior_weight: float = 0.0, keep_best: bool = True,
                 graphed: bool = True):
        if isinstance(steps, bool) or not isinstance(steps, int) or steps < 0:
            raise ValueError("steps must be an integer >= 0")
        self.steps = steps
        self.lr = _finite_nonneg("lr", lr)
        try:
            b1, b2 = (float(b) for b in betas)
        except (TypeError, ValueError):
            raise ValueError("betas must be two numbers in [0, 1)") from None
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError("betas must be two numbers in [0, 1)")
        self.betas = (b1, b2)
        self.eps = _finite_nonneg("eps", eps)
        self.alpha_adv = _finite_nonneg("alpha_adv", alpha_adv)
        self.prior_weight = _finite_nonneg("prior_weight", prior_weight)
        for name, flag in (("keep_best", keep_best), ("graphed", graphed)):
            if not isinstance(flag, bool):
                raise ValueError(f"{name} must be True or False")
        self.keep_best, self.graphed = keep_best, graphed
        if self.alpha_adv != 0.0 and discriminator is None:
            raise ValueError("alpha_adv != 0 needs a discriminator")
        nets = [n for n in (encoder, decoder, discriminator) if n is not None]
        if len({n._dt for n in nets}) != 1:
            raise ValueError("encoder / decoder / discriminator must share one engine dtype")
        if encoder is not None and (decoder.nz != encoder.latent_dim or decoder.img_size != encoder._img or
                                    decoder.nc != encoder._engine.in_ch):
            raise ValueError("LatentRefiner needs a Generator that decodes the Encoder's latent into the Encoder's image shape")
        if discriminator is not None and (discriminator.nc != decoder.nc or discriminator.img_size != decoder.img_size):
            raise ValueError("LatentRefiner needs a Discriminator of the Generator's image shape")
        # a Discriminator without an adversarial weight has no term in J: it is not run
        self.E, self.G, self.D = encoder, decoder, discriminator if self.alpha_adv != 0.0 else None
        self.dt, self.latent = decoder._dt, decoder.nz
        self._bufs = {}                     # B -> the static buffers of that batch size
        self._caps = {}                     # B -> capture.Captured of one iteration
        self.captures = 0                   # captures made so far (a replayed call adds none)

    # ---- pieces of one iteration ------------------------------------------------------------------------------------
    def _buffers(self, B: int, dev):
        buf = self._bufs.get(B)
        if buf is None or buf["noisy"].device != dev:
            Gn, dt = self.G, self.dt
            f32 = dict(dtype=torch.float32, device=dev)
            buf = dict(state=ops.latent_state(B, self.latent, dev),
                       z_eng=ops.empty_act((B, 1, 1, G.padc(Gn.nz, dt)), dt, dev),
                       noisy=torch.empty(B, Gn.nc, Gn.img_size, Gn.img_size, **f32), rects=torch.empty(B, 8, **f32),
                       loss_rows=torch.empty(B, **f32), objective=torch.empty(B, **f32), objective0=torch.empty(B, **f32),
                       slot=torch.empty(1, **f32))
            self._bufs[B] = buf
            self._caps.pop(B, None)
        return buf

    def _evaluate(self, buf, B: int, want_grad: bool):
        """G(z_eng), the context loss rows against the static input and, with a Discriminator, its probabilities.
        -> (recon NCHW f32, G's context, d loss / d recon or None, p or None, D's context)"""
        Gn, D, dt = self.G, self.D, self.dt
        CP = G.padc(Gn.nc, dt)
        d_in = None
        if Gn.fused_tail(B):
            tail = {}
            if D is not None:               # the last layer's kernel writes the image in D's layout as well (no noise added)
                d_in = ops.empty_act((B, Gn.img_size, Gn.img_size, CP), dt, buf["noisy"].device)
                tail = dict(out_noisy=d_in)
            recon, ctxG = Gn._engine.forward(buf["z_eng"], B, False, keep=want_grad, tail=tail)
        else:
            pre, ctxG = Gn._engine.forward(buf["z_eng"], B, False, keep=want_grad)
            recon = ops.nhwc_to_nchw(pre, Gn.nc, dt, apply_tanh=True)
            if D is not None:
                d_in = ops.nchw_to_nhwc(recon, CP, dt)
        d_recon = ops.masked_mse_rows(recon, buf["noisy"], buf["rects"], 1.0, buf["loss_rows"], want_grad)
        p = ctxD = None
        if D is not None:
            p, ctxD = D._engine.forward(d_in, B, False, keep=want_grad)
        return recon, ctxG, d_recon, p, ctxD

    def _iterate(self, buf, B: int) -> None:
        """One refinement iteration on the static buffers; no host value, no allocation outside torch's allocator."""
        Gn, D, dt = self.G, self.D, self.dt
        recon, ctxG, d_recon, p, ctxD = self._evaluate(buf, B, True)
        sink = GradSink(direct=False)       # never asked: no parameter gradient is formed
        CP = G.padc(Gn.nc, dt)
        if D is not None:
            # gradient scale alpha_adv * B against the launch's 1 / B: every image gets the gradient of ITS term
            gscale = self.alpha_adv * B
            if B <= ops.HEAD_BWD_MAXROWS and D._engine.stages[-1].kind == "head":
                d_img = D._engine.backward(ctxD, None, True, sink, param_grads=False,
                                           head_loss=(self.REAL_LABEL, 0.0, 1, gscale, buf["slot"], False))
            else:
                dp = ops.bce_forward_backward(p, self.REAL_LABEL, gscale, buf["slot"], False, True)
                d_img = D._engine.backward(ctxD, dp, True, sink, param_grads=False)
            d_pre = ops.nchw_grad_add_to_nhwc(d_recon, d_img, recon, CP, dt)     # both image gradients, through Tanh
        else:
            d_pre = ops.nchw_grad_to_nhwc(d_recon, recon, CP, dt)
        dz = Gn._engine.backward(ctxG, d_pre, True, sink, param_grads=False)
        ops.latent_adam("update", buf["state"], dt, buf["z_eng"].shape[-1], dz=dz, loss_rows=buf["loss_rows"], p=p,
                        z_out=buf["z_eng"], objective=buf["objective"], lr=self.lr, betas=self.betas, eps=self.eps,
                        alpha_adv=self.alpha_adv, prior_weight=self.prior_weight)

    def _engines(self):
        return [n._engine for n in (self.G, self.D) if n is not None]

    def _capture_key(self, B: int):
        """The batch size and, per engine in the iteration, what its packed operands are valid for and where they live."""
        for e in self._engines():
            e._ensure_packed()              # the weights are constants of the loop: packed before, never inside, a capture
        return (B,) + tuple((e.pack_key(), e._pack_ptrs, id(e._packs)) for e in self._engines())

    # ---- the public call ----------------------------------------------------------------------------------------------
    @torch.no_grad()
    def refine(self, noisy: torch.Tensor, rects: Optional[torch.Tensor] = None, init="mu",
               eps_z: Optional[torch.Tensor] = None) -> Dict[str, object]:
        """noisy: f32 [B,C,S,S] on the MI355X in [-1,1], the degraded input.  rects: f32 [B, 8] in ops.degrade_params' layout
        (``DeviceLoader.last_rects``), the occlusion rectangle of each image -- excluded from the context loss; None: no holes.
        init: "mu" (z0 = the Encoder's mean), "sample" (z0 = mu + exp(logvar / 2) * eps_z; eps_z f32 [B, L] injects the draw,
        else it comes from the device noise stream) or an f32 [B, L] device tensor.
        Returns device tensors: recon (NCHW f32, decoded from z), z [B, L] f32 (the best iterate with keep_best, else the
        last), z0, recon0 (the one-shot reconstruction from z0), objective0 and objective ([B] each: J at z0 and at z), and
        steps (int).  No host synchronisation (the first call of a batch size under graphed=True captures, which has one)."""
        what = "LatentRefiner.refine"
        E, Gn, dt = self.E, self.G, self.dt
        if not isinstance(noisy, torch.Tensor) or not noisy.is_cuda:
            raise RuntimeError(f"{what} needs the batch on the MI355X ('cuda'); there is no CPU path")
        if noisy.dim() != 4 or noisy.dtype != torch.float32 or tuple(noisy.shape[1:]) != (Gn.nc, Gn.img_size, Gn.img_size):
            raise RuntimeError(f"{what}: noisy must be float32 [B,{Gn.nc},{Gn.img_size},{Gn.img_size}]")
        B, L, dev = noisy.shape[0], self.latent, noisy.device
        if rects is not None and (not rects.is_cuda or rects.dtype != torch.float32 or tuple(rects.shape) != (B, 8)):
            raise RuntimeError(f"{what}: rects must be a device f32 [B, 8] tensor (ops.degrade_params)")
        if isinstance(init, str) and init not in ("mu", "sample"):
            raise ValueError(f"{what}: init must be 'mu', 'sample' or an f32 [B, L] device tensor, got {init!r}")
        if not isinstance(init, str) and not (isinstance(init, torch.Tensor) and init.is_cuda and
                                              init.dtype == torch.float32 and tuple(init.shape) == (B, L)):
            raise ValueError(f"{what}: init must be 'mu', 'sample' or an f32 [B, L] device tensor")
        if isinstance(init, str) and E is None:
            raise ValueError(f"{what}: a refiner built without an encoder needs init= an f32 [B, L] device tensor")
        if eps_z is not None:
            if not (isinstance(init, str) and init == "sample"):
                raise ValueError(f"{what}: eps_z belongs to init='sample'")
            if not eps_z.is_cuda or eps_z.dtype != torch.float32 or tuple(eps_z.shape) != (B, L):
                raise RuntimeError(f"{what}: eps_z must be a device f32 [{B}, {L}] tensor")
        ZP = G.padc(Gn.nz, dt)
        buf = self._buffers(B, dev)
        st = buf["state"]
        buf["noisy"].copy_(noisy)
        if rects is None:
            buf["rects"].fill_(float("nan"))            # a NaN row: no comparison holds, that image has no hole
        else:
            buf["rects"].copy_(rects)
        # ---- z0 in the engine layout ----
        if isinstance(init, str):
            noisy_h = ops.nchw_to_nhwc(buf["noisy"], G.padc(Gn.nc, dt), dt)
            mulv, _ = E._engine.forward(noisy_h, B, False, keep=False)
            if init == "mu":
                eps_z = ops.zeros_f32(B * L, dev).view(B, L)
            elif eps_z is None:
                eps_z = _default_draws(dev, None, (B, L))[1]
            z0_eng, _ = ops.reparam_forward(mulv.view(B, -1), eps_z.contiguous(), L, ZP, dt)
        else:
            z0_eng = ops.prior_forward(init.contiguous(), B, L, ZP, dt)

        def start():
            ops.latent_adam("init", st, dt, ZP, z_in=z0_eng, z_out=buf["z_eng"])

        cap = None
        if self.graphed and self.steps > 0:
            key = self._capture_key(B)
            cap = self._caps.get(B)
            if cap is None or cap.key != key:
                start()
                self._iterate(buf, B)                   # eager warm-up: the workspaces reach their size outside the capture
                cap = capture(lambda: self._iterate(buf, B), [], HostMirrors([], []), dev, key=key, keep=buf)
                self._caps[B] = cap
                self.captures += 1
        start()
        z0 = st["z"].clone()
        recon0 = Gn.decode_eval(buf["z_eng"], B)
        for k in range(self.steps):                     # no host value inside: `steps` launches sequences / replays in a row
            if cap is not None:
                replay(cap)
            else:
                self._iterate(buf, B)
            if k == 0:
                buf["objective0"].copy_(buf["objective"])
        # the last iterate's objective (the loop evaluated every iterate but the one its last step produced)
        _, _, _, p, _ = self._evaluate(buf, B, False)
        ops.latent_adam("track", st, dt, ZP, loss_rows=buf["loss_rows"], p=p, objective=buf["objective"],
                        alpha_adv=self.alpha_adv, prior_weight=self.prior_weight)
        if self.steps == 0:
            buf["objective0"].copy_(buf["objective"])
        z = (st["best_z"] if self.keep_best else st["z"]).clone()
        objective = (st["best_loss"] if self.keep_best else buf["objective"]).clone()
        recon = Gn.decode_eval(ops.prior_forward(z, B, L, ZP, dt), B)
        return {"recon": recon, "z": z, "z0": z0, "recon0": recon0, "objective0": buf["objective0"].clone(),
                "objective": objective, "steps": self.steps}


@torch.no_grad()
def denoise_tiled(encoder, decoder, images, *, stride: Optional[int] = None, window: str = "hann", batch: int = 128,
                  sample: bool = True, eps_z: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Denoise images LARGER than the networks (not in the reference, whose networks take S x S only): cut every image into
    overlapping S x S tiles (``tiling.tile_plan``: origins every ``stride``, default S // 2, the last tile flush with the
    edge, no padding), run Encoder -> reparameterise -> Generator on chunks of at most ``batch`` tiles, and blend the
    reconstructions with a separable ``window`` ("hann" | "tri" | "box") whose normalised coefficients the plan holds.
    images: f32 [N,C,H,W] on the MI355X in [-1,1], or the resident uint8 set (``data.ResidentImages``, or a uint8 [N,H,W,C]
    tensor / slice of one), normalised as ``ResidentImages.batch`` does.  Returns f32 [N,C,H,W].
    Both networks are put in eval mode (as validation_epoch does): BatchNorm then does not depend on how the tiles fall into
    chunks.  sample=True draws the reparameterisation noise per tile from the device noise stream (the reference's behaviour
    per image); sample=False uses z = mu; eps_z f32 [N * ny * nx, latent_dim] injects the draws (tile t = (n * ny + ky) * nx + kx).
    Per chunk: ops.tile_gather -> the two engines -> ops.nhwc_to_nchw(tanh) into its slice of the tile buffer; then ONE
    ops.tile_blend launch.  No host synchronisation inside."""
    if isinstance(images, torch.Tensor):
        src = images
    elif isinstance(getattr(images, "images", None), torch.Tensor):
        src = images.images
    else:
        raise RuntimeError("denoise_tiled: images must be a device tensor or a resident uint8 set")
    if not src.is_cuda:
        raise RuntimeError("denoise_tiled needs the images on the MI355X ('cuda'); there is no CPU path")
    if src.dim() != 4 or src.dtype not in (torch.uint8, torch.float32):
        raise RuntimeError("denoise_tiled: images must be float32 [N,C,H,W] or uint8 [N,H,W,C]")
    src = src.contiguous()
    u8 = src.dtype == torch.uint8
    N, H, W, C = src.shape if u8 else (src.shape[0], src.shape[2], src.shape[3], src.shape[1])
    S, dt, L = encoder._img, encoder._dt, encoder.latent_dim
    if decoder.img_size != S or decoder._dt != dt or decoder.nc != C:
        raise RuntimeError("denoise_tiled: encoder, decoder and images disagree on the tile size, dtype or channel count")
    if int(batch) < 1 or N < 1:
        raise RuntimeError("denoise_tiled: batch and the number of images must be at least 1")
    plan = tiling.cached_plan(H, W, S, stride, window)
    T = N * plan.tiles_per_image
    dev = src.device
    if eps_z is not None:
        if not eps_z.is_cuda or eps_z.dtype != torch.float32 or tuple(eps_z.shape) != (T, L):
            raise RuntimeError(f"denoise_tiled: eps_z must be a device f32 [{T}, {L}] tensor (one row per tile)")
        eps_z = eps_z.contiguous()
    elif sample:
        eps_z = _default_draws(dev, None, (T, L))[1]
    else:
        eps_z = ops.zeros_f32(T * L, dev).view(T, L)     # z = mu
    encoder.eval(), decoder.eval()
    tiles = torch.empty(T, C, S, S, dtype=torch.float32, device=dev)
    for t0 in range(0, T, int(batch)):
        b = min(int(batch), T - t0)
        x = ops.tile_gather(src, plan, t0, b, G.padc(C, dt), dt)
        _reconstruct(encoder, decoder, x, b, eps_z[t0:t0 + b], out=tiles[t0:t0 + b])
    return ops.tile_blend(tiles, plan)


def _tile_count(encoder, img, tiling_kw) -> int:
    plan = tiling.cached_plan(img.shape[2], img.shape[3], encoder._img, tiling_kw.get("stride"), tiling_kw.get("window", "hann"))
    return img.shape[0] * plan.tiles_per_image


@torch.no_grad()
def tiled_denoise_eval(encoder, decoder, img: torch.Tensor, sigma: float = 0.05, eps: Optional[torch.Tensor] = None,
                       noisy: Optional[torch.Tensor] = None, ms_ssim: bool = False, **tiling_kw) -> Dict[str, object]:
    """denoise_eval at full resolution.  img: f32 [N,C,H,W] on the MI355X in [-1,1], H, W >= the networks' S.  The noise is
    added ONCE to the whole image, noisy = clamp(img + sigma*eps, -1, 1) (eps: injected draws of img's shape, else generated
    on the device), so overlapping tiles see the same noisy pixel; ``noisy`` given: used instead, sigma / eps ignored.  Then
    ``denoise_tiled(encoder, decoder, noisy, **tiling_kw)`` (stride, window, batch, sample, eps_z).
    Returns noisy, recon (NCHW f32) and python floats: recon_loss (mean squared error of recon vs img), psnr, ssim, and
    noisy_loss, psnr_noisy, ssim_noisy of the input, all on the H x W tensors ([0,1]-rescaled for PSNR / SSIM, as
    denoise_eval), plus tiles.  One host sync.  ms_ssim=True (default False: nothing changes) adds ``ms_ssim`` and
    ``ms_ssim_noisy`` (ops.ms_ssim on the H x W tensors, the default scales of that size), read in the same sync."""
    if not img.is_cuda:
        raise RuntimeError("tiled_denoise_eval needs the batch on the MI355X ('cuda'); there is no CPU path")
    if img.dim() != 4 or img.dtype != torch.float32:
        raise RuntimeError("tiled_denoise_eval: img must be float32 [N,C,H,W]")
    img = img.contiguous()
    dt = encoder._dt
    if noisy is not None:
        if not noisy.is_cuda or noisy.shape != img.shape:
            raise RuntimeError("tiled_denoise_eval: noisy must be a device batch of img's shape")
        noisy = noisy.contiguous()
    else:
        if eps is None:
            eps = _default_draws(img.device, img.shape, None)[0]
        _, noisy = ops.noisy_clamp_to_nhwc(img, eps, sigma, G.padc(img.shape[1], dt), dt)
    recon = denoise_tiled(encoder, decoder, noisy, **tiling_kw)
    qs = [_Quality("", ms_ssim), _Quality("_noisy", ms_ssim)]
    sums = _allocate(img.device, 0, qs)
    for q, x in zip(qs, (recon, noisy)):
        q.update(x, img, 1, store=True)                  # the one batch of this pass, weight 1
    return {"noisy": noisy, "recon": recon, **_tiled_eval_result(qs, _read(sums, qs), _tile_count(encoder, img, tiling_kw))}


def _tiled_eval_result(qs, host, tiles: int) -> Dict[str, float]:
    """Host only.  host: tiled_denoise_eval's read, the slots of the reconstruction and of the noisy input (one batch: seen = 1)."""
    r, noisy = _results(qs, host, 0, 1)
    out = {"recon_loss": r[0]["recon_loss"], "psnr": r[0]["psnr"], "ssim": r[0]["ssim"], "noisy_loss": noisy[0]["recon_loss_noisy"],
           "psnr_noisy": noisy[0]["psnr_noisy"], "ssim_noisy": noisy[0]["ssim_noisy"], "tiles": tiles}
    return _add_optional(out, (r, noisy))


@torch.no_grad()
def tiled_test_epoch(encoder, decoder, pairs: Iterable, ms_ssim: bool = False, baseline=None, **tiling_kw) -> Dict[str, float]:
    """paired_test_epoch at full resolution: ``pairs`` yields (noisy, clean) device batches f32 [b,C,H,W] in [-1,1], each
    denoised with ``denoise_tiled(encoder, decoder, noisy, **tiling_kw)``.  Accumulation stays on the device (per batch the
    mean squared error and the mean SSIM, weighed by the batch's image count); ONE host sync at the end.  Returns python
    floats: psnr, ssim, recon_loss (mean squared error per element) of recon vs clean, psnr_noisy, ssim_noisy of the input,
    samples, tiles.  ms_ssim=True (default False: nothing changes) adds ``ms_ssim`` and ``ms_ssim_noisy`` (ops.ms_ssim, the
    default scales of the image size), accumulated like ssim and read in the same sync.
    baseline (default None: nothing changes): as in paired_test_epoch, a ``baselines.NLMeans``, "nlm" or a dict of its keywords;
    here there are whole large images and no loader, so the noise level is ``sigma="estimate"`` (what "nlm" means here) or a
    number -- "oracle" is refused.  The filter runs on the full H x W image, no tiling, and the result gains ``recon_loss_nlm``,
    ``ssim_nlm``, ``psnr_nlm`` (and ``ms_ssim_nlm`` with ms_ssim=True), read in the same sync.  A ``baselines.Median``, "median" or
    ``{"radius": r}``: the median filter, keys suffixed ``_median``."""
    nlm = make_baseline("tiled_test_epoch", baseline, allow_oracle=False)
    qs = [_Quality("", ms_ssim), _Quality("_noisy", ms_ssim)] + ([_Quality("_" + nlm.name, ms_ssim)] if nlm is not None else [])
    sums, seen, tiles = None, 0, 0
    for noisy, clean in pairs:
        if not (noisy.is_cuda and clean.is_cuda):
            raise RuntimeError("tiled_test_epoch needs device pairs; there is no CPU path")
        sums = _allocate(clean.device, 0, qs) if sums is None else sums
        if noisy.shape != clean.shape or clean.dim() != 4:
            raise RuntimeError("tiled_test_epoch: noisy and clean must be [b,C,H,W] batches of one shape")
        noisy, clean = noisy.contiguous(), clean.contiguous()
        b = clean.shape[0]
        candidates = [denoise_tiled(encoder, decoder, noisy, **tiling_kw), noisy] + ([nlm(noisy)] if nlm is not None else [])
        for q, x in zip(qs, candidates):
            q.update(x, clean, b)
        seen += b
        tiles += _tile_count(encoder, clean, tiling_kw)
    if seen == 0:
        raise RuntimeError("tiled_test_epoch: pairs yielded no batch")
    return _tiled_test_result(qs, _read(sums, qs), seen, tiles)


def _tiled_test_result(qs, host, seen: int, tiles: int) -> Dict[str, float]:
    """Host only.  host: tiled_test_epoch's read, the slots of the reconstruction, the noisy input and, if the pass had one,
    the baseline."""
    r, noisy, *further = _results(qs, host, 0, seen)
    out = {"psnr": r[0]["psnr"], "ssim": r[0]["ssim"], "recon_loss": r[0]["recon_loss"], "psnr_noisy": noisy[0]["psnr_noisy"],
           "ssim_noisy": noisy[0]["ssim_noisy"], "samples": seen, "tiles": tiles}
    return _add_optional(out, (r, noisy), further)
