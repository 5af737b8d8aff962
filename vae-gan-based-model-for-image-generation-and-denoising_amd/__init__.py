"""MI355X-native VAE-GAN training path.  Importable as ``vaegan_amd`` through the alias
module at the repository root (this directory's name is not a Python identifier).

Drop-in surface: ``Encoder``, ``ConvBlock`` (main_vae.py:20-58), ``Generator``,
``Discriminator``, ``weights_init`` (gan_code.py:16-97), ``Adam`` (torch.optim.Adam as used at
vaegan_code.py:42-44), ``BCELoss`` / ``MSELoss`` (vaegan_code.py:46-47), ``configure_seed``
(utils.py:6-14), ``VAEGANTrainer`` (the loop body of vaegan_code.py:65-135) and ``graphed`` (hipGraph replay of a
reference-shaped step function).  The learned-similarity term of Larsen et al. (the reference README's eq. 2, absent from
its code): ``VAEGANTrainer(..., feat_layer=, alpha_feat=, alpha_pix=)`` and ``Discriminator.features(x, layer)`` /
``Discriminator.feature_layers()``.  The SSIM reconstruction loss (1 - the SSIM the denoising passes report; not in the
reference): ``SSIMLoss`` and ``VAEGANTrainer(..., alpha_ssim=)`` / ``VAETrainer(..., alpha_ssim=)``; its multi-scale form (MS-SSIM over a 2x
pyramid): ``MSSSIMLoss``, ``msssim_weights``, ``ssim_scales=`` on the two trainers and ``ms_ssim=True`` on the denoising passes.  Generation (main_vae.py:415-641): ``latent`` -- ``encode_dataset``, ``LatentPrior``,
``evaluate_generation``, ``sample_images``, and ``GaussianMixturePrior`` (not in the reference): a full-covariance Gaussian
mixture fitted to the Encoder's latents by EM on the device and sampled there, a drop-in ``prior=``.  Feature-space metrics (fid.update / fid.compute of every evaluation loop,
README.md:22 precision / recall): ``metrics`` -- ``FeatureStats``, ``frechet_distance``, ``precision_recall``,
``encoder_features``, ``kernel_distance`` (KID), ``ndb`` (number of statistically different bins over k-means bins of the
real features; no classifier needed; ``evaluate_generation_ndb`` adds it to a generation pass).  K-means on the device (not in the reference): ``cluster`` -- ``KMeans`` (Lloyd's
iteration with k-means++ seeding), also the k-means start of ``GaussianMixturePrior.fit(init="kmeans")``.  Weight averaging (not in the reference): ``EMA`` -- an exponential moving
average of Encoder / Generator weights kept on the device, ``VAEGANTrainer(..., ema=)`` and the sibling trainers.
Gradient-norm clipping (not in the reference): ``clip_grad_norm_`` / ``Adam.clip_grad_norm_`` -- torch's
``clip_grad_norm_`` with the coefficient kept on the device and applied inside the Adam step, ``max_grad_norm=`` on the four
trainers.  Differentiable augmentation of the Discriminator's inputs (not in the reference): ``DiffAugment`` and
``augment=`` on the three adversarial trainers.  Learning-rate schedules and decoupled weight decay (not in the reference):
``LRSchedule`` (``Adam(..., lr_schedule=)``: warm-up and linear / cosine / exponential / step decay, evaluated on the device from
the step count, so a captured iteration replays a moving rate) and ``AdamW``.  Data path (dataset_code.py): ``data`` -- ``ResidentImages`` (``resized``: Resize +
CenterCrop on the device), ``resample_coeffs``, ``resize_geometry``.  Tiled denoising of images larger than the networks
(not in the reference): ``denoise_tiled``, ``tiled_denoise_eval``, ``tiled_test_epoch`` and ``tiling`` -- ``tile_plan`` /
``TilePlan``: overlapping S x S tiles cut and blended back on the device with a separable window.  Test-time latent
refinement (not in the reference; GAN-inversion denoising / inpainting): ``LatentRefiner`` -- Adam on the latent of the frozen
networks against the input outside its occlusion rectangle, and ``paired_test_epoch(..., refine=)``.  Classical-denoiser
baseline (not in the reference): ``NLMeans`` (``baselines``) -- non-local means on the device with the loader's own or a
blindly estimated noise level (``ops.nlm_denoise``, ``ops.noise_sigma``), ``Median`` -- the (2r+1)^2 median filter
(``ops.median_filter``), and ``baseline=`` on ``paired_test_epoch`` / ``tiled_test_epoch``.  Noise models of the degraded
pairs (not in the reference): ``data.Degrade(noise_model="gaussian" | "speckle" | "shot", impulse_max_p=, salt_ratio=)``.
Spectral generation metric (not in the reference for images): ``spectrum`` -- ``spectrum_plan`` / ``SpectrumPlan``, the
windowed DFT tables and radial bins of an image size; ``SpectrumStats`` and ``spectral_distance`` (``metrics``): running
radially binned power spectra on the device (``ops.spectrum_profiles``, ``ops.spectrum_accum``, f64 MFMA) and the log-spectral
distance / high-frequency share of two image sets; ``evaluate_generation_spectrum`` adds them to a generation pass.
"""
from . import baselines  # noqa: F401
from . import cluster  # noqa: F401
from . import data  # noqa: F401
from . import geometry  # noqa: F401
from . import latent  # noqa: F401
from . import metrics  # noqa: F401
from .data import ResidentImages, resample_coeffs, resize_geometry
from .augment import DiffAugment
from .baselines import Median, NLMeans
from .ddp import GradReducer
from .ema import EMA
from . import tiling  # noqa: F401
from .denoise import (LatentRefiner, denoise_eval, denoise_tiled, paired_test_epoch, tiled_denoise_eval, tiled_test_epoch,
                      validation_epoch)
from .tiling import TilePlan, tile_plan
from .graphed import graphed
from . import spectrum  # noqa: F401
from .latent import (GaussianMixturePrior, LatentPrior, encode_dataset, evaluate_generation, evaluate_generation_ndb,
                     evaluate_generation_spectrum, sample_images)
from .cluster import KMeans
from .metrics import (FeatureStats, SpectrumStats, encoder_features, frechet_distance, kernel_distance, ndb,
                      precision_recall, spectral_distance)
from .losses import BCELoss, MSELoss, MSSSIMLoss, SSIMLoss, msssim_weights
from .nets import ConvBlock, Discriminator, Encoder, Generator, weights_init
from .optim import Adam, AdamW, LRSchedule, clip_grad_norm_
from .siblings import DCGANTrainer, VAETrainer, WGANTrainer
from .trainer import LOSS_NAMES, VAEGANTrainer
from .utils import configure_seed

__all__ = ["ConvBlock", "Encoder", "Generator", "Discriminator", "weights_init", "Adam", "BCELoss", "MSELoss", "SSIMLoss",
           "VAEGANTrainer", "LOSS_NAMES", "configure_seed", "geometry", "denoise_eval", "validation_epoch", "paired_test_epoch", "GradReducer", "data", "VAETrainer", "DCGANTrainer", "WGANTrainer", "graphed",
           "latent", "LatentPrior", "GaussianMixturePrior", "encode_dataset", "evaluate_generation", "sample_images",
           "ResidentImages", "resample_coeffs", "resize_geometry",
           "EMA", "clip_grad_norm_", "DiffAugment", "AdamW", "LRSchedule",
           "tiling", "TilePlan", "tile_plan", "denoise_tiled", "tiled_denoise_eval", "tiled_test_epoch",
           "metrics", "FeatureStats", "frechet_distance", "precision_recall", "encoder_features", "kernel_distance",
           "cluster", "KMeans", "ndb", "evaluate_generation_ndb", "MSSSIMLoss", "msssim_weights", "LatentRefiner",
           "baselines", "NLMeans", "Median",
           "spectrum", "SpectrumStats", "spectral_distance", "evaluate_generation_spectrum"]
