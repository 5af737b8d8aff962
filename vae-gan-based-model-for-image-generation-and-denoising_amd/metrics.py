"""Feature-space generation metrics on the device: FID, the k-nearest-neighbour precision / recall / F1, KID and NDB.

Every evaluation loop of the reference ends in ``fid.update(real, real=True); fid.update(fake, real=False); fid.compute()``
(vaegan_code.py:143-185, gan_code.py:111-145, main_vae.py:472-512, :540-574), and its README.md:22 lists Precision /
Recall / F1 "computed via manifold distances" (Kynkaanniemi et al. 2019, "Improved Precision and Recall Metric for
Assessing Generative Models"), which the reference implements nowhere.  This module is everything AFTER a feature vector
exists; the three kernels behind it are stated in include/vaegan_hip.h, "Feature-space metrics":

    FeatureStats.update      vg_feat_stats_accum   f64 running sums (sum x, sum x x^T) on the f64 MFMA
    precision_recall         vg_knn_radius2        k-th neighbour radius of every sample, exact-f32 MFMA
                             vg_manifold_cover     is a sample inside some ball of the other set
    kernel_distance          vg_kid_scores         polynomial-kernel MMD^2 over random subsets (KID), f64 MFMA
    ndb                      vg_kmeans_*           k-means bins of the real features (cluster.KMeans), the fake rows' bin counts

The feature extractor is pluggable: ``feature_fn(images_u8 [b,C,S,S] uint8 device) -> f32 [b, D] device``.
``encoder_features`` wraps the project's own Encoder (no download); a user who has InceptionV3 weights passes a callable of
their own and gets the reference's FID.  This module never imports a network, so Inception Score stays out of scope.
Parity with the torchmetrics package itself is unpinned (the package is not installed), as for SSIM: the formulas are
torchmetrics' ``_compute_fid`` and running sums, checked against an f64 numpy restatement (tests/_metrics_ref.py).
Precision / recall is single-process: ``FeatureStats.merge`` makes the FID side additive over ranks, the k-NN part needs
all features in one place.  So is the Kernel Inception Distance (Binkowski et al. 2018, "Demystifying MMD GANs"), which
the reference computes nowhere either: it is the unbiased companion of FID for small validation sets (FID's estimator is
biased in N).  Deviations from torchmetrics' KernelInceptionDistance, whose parity is unpinned for the
same reason: the subsets are drawn on the HOST by numpy's PCG64 (``kid_subsets``), the arithmetic is f64 and ``kid_std``
is the population standard deviation (torch.std's default is the sample one).
"""
import math
from typing import Callable, Dict, Optional

import numpy as np
import torch

from . import ops
from .cluster import KMeans


def _check_feats(f, D: Optional[int], what: str) -> None:
    if not isinstance(f, torch.Tensor) or not f.is_cuda:
        raise RuntimeError(f"{what} needs features on the MI355X ('cuda'); there is no CPU path")
    if f.dtype != torch.float32 or f.dim() != 2 or (D is not None and f.shape[1] != D):
        raise RuntimeError(f"{what}: features must be f32 [b, {'D' if D is None else D}], got {f.dtype} {tuple(f.shape)}")


class FeatureStats:
    """Running first and second moments of a feature stream, as torchmetrics' FrechetInceptionDistance keeps them:
    ``sum`` f64 [D] (features.double().sum(0)), ``outer`` f64 [D, D] (features.double().T @ features.double()) and the
    row count ``n`` (a python int: batch sizes are known on the host, no sync).  ``update`` runs on the device and is
    deterministic; a FeatureStats on the CPU only HOLDS state (``load_state_dict`` of a saved one, ``frechet_distance``)."""

    def __init__(self, D: int, device="cuda"):
        D = int(D)
        if not 1 <= D <= 2048:
            raise RuntimeError(f"FeatureStats: the feature dimension must be in [1, 2048], got {D}")
        self.D, self.n = D, 0
        self.sum = torch.zeros(D, dtype=torch.float64, device=device)
        self.outer = torch.zeros(D, D, dtype=torch.float64, device=device)

    def update(self, feats: torch.Tensor) -> "FeatureStats":
        """feats f32 [b, D] on the device, any b >= 0 (ragged batches).  No host sync."""
        if not self.sum.is_cuda:
            raise RuntimeError("FeatureStats.update needs the statistics on the MI355X ('cuda'); there is no CPU path")
        _check_feats(feats, self.D, "FeatureStats.update")
        ops.feat_stats_accum(feats, self.sum, self.outer)
        self.n += int(feats.shape[0])
        return self

    def merge(self, other: "FeatureStats") -> "FeatureStats":
        """Add another stream's sums (another rank's, another shard's): the statistics are additive."""
        if other.D != self.D:
            raise RuntimeError(f"FeatureStats.merge: feature dimensions differ ({self.D} vs {other.D})")
        self.sum += other.sum.to(self.sum.device)
        self.outer += other.outer.to(self.outer.device)
        self.n += other.n
        return self

    def _host(self):
        return self.sum.cpu().numpy(), self.outer.cpu().numpy()

    def mean(self) -> np.ndarray:
        """sum / n as a host f64 array [D] (one copy of D doubles)."""
        if self.n < 1:
            raise RuntimeError("FeatureStats.mean: no sample yet")
        return self.sum.cpu().numpy() / self.n

    def cov(self) -> np.ndarray:
        """(outer - n m m^T) / (n - 1), f64, as torchmetrics; a host array [D, D] (one copy of D + D^2 doubles)."""
        if self.n < 2:
            raise RuntimeError("FeatureStats.cov needs at least two samples")
        s, o = self._host()
        m = s / self.n
        return (o - self.n * np.outer(m, m)) / (self.n - 1)

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """Plain tensors: compute the real side once per data set, save it, reuse it for every checkpoint."""
        return {"sum": self.sum, "outer": self.outer, "n": torch.tensor(self.n, dtype=torch.int64)}

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> "FeatureStats":
        s, o = sd["sum"], sd["outer"]
        if (s.dtype != torch.float64 or o.dtype != torch.float64 or tuple(s.shape) != (self.D,)
                or tuple(o.shape) != (self.D, self.D)):
            raise RuntimeError(f"FeatureStats: sum must be f64 [{self.D}] and outer f64 [{self.D},{self.D}]")
        dev = self.sum.device
        self.sum, self.outer, self.n = s.to(dev).contiguous().clone(), o.to(dev).contiguous().clone(), int(sd["n"])
        return self


def frechet_distance(real: FeatureStats, fake: FeatureStats) -> float:
    """torchmetrics' ``_compute_fid`` on two sets of running statistics:

        |m1 - m2|^2 + tr S1 + tr S2 - 2 sum Re sqrt(eigvals(S1 S2))

    The sums were accumulated on the device in f64; this last D x D step (mean, covariance, the eigenvalues of a
    non-symmetric product) runs on the HOST in numpy f64: one copy of 2 (D + D^2) doubles per evaluation pass and the only
    host work of the metric.  A device eigensolver is deliberately out of scope."""
    if real.D != fake.D:
        raise RuntimeError(f"frechet_distance: feature dimensions differ ({real.D} vs {fake.D})")
    if real.n < 2 or fake.n < 2:
        raise RuntimeError("frechet_distance needs at least two samples on each side")
    m1, m2 = real.mean(), fake.mean()
    s1, s2 = real.cov(), fake.cov()
    d = m1 - m2
    c = np.sqrt(np.linalg.eigvals(s1 @ s2).astype(np.complex128)).real.sum()
    return float(d @ d + np.trace(s1) + np.trace(s2) - 2.0 * c)


class SpectrumStats:
    """Running binned power spectra of an image stream, the twin of ``FeatureStats`` for the spectral metric (not in the
    reference for images; it compares mean Welch PSDs of real and generated EEG, test_eegglow.py:25-46): ``sum`` and
    ``sumsq`` f64 [n_bins] of the per-image profiles of ``plan`` (a ``spectrum.SpectrumPlan``) and the image count ``n`` (a
    python int).  ``update`` runs on the device (vg_spectrum_profiles, vg_spectrum_accum) and is deterministic; an instance
    on the CPU only HOLDS state.  No network is involved: the metric sees the top octave that every feature space built on
    strided convolutions throws away."""

    def __init__(self, plan, device="cuda", center: bool = True):
        from .spectrum import SpectrumPlan
        if not isinstance(plan, SpectrumPlan):
            raise RuntimeError("SpectrumStats: plan must be a spectrum.SpectrumPlan (spectrum.spectrum_plan(H, W))")
        if not isinstance(center, bool):
            raise RuntimeError("SpectrumStats: center must be a bool")
        self.plan, self.center, self.n = plan, center, 0
        self.sum = torch.zeros(plan.n_bins, dtype=torch.float64, device=device)
        self.sumsq = torch.zeros(plan.n_bins, dtype=torch.float64, device=device)

    def update(self, images: torch.Tensor) -> "SpectrumStats":
        """images f32 [b, C, H, W] on the device, any b >= 0 (ragged batches).  No host sync."""
        if not self.sum.is_cuda:
            raise RuntimeError("SpectrumStats.update needs the statistics on the MI355X ('cuda'); there is no CPU path")
        if not isinstance(images, torch.Tensor) or not images.is_cuda:
            raise RuntimeError("SpectrumStats.update needs images on the MI355X ('cuda'); there is no CPU path")
        if images.dtype != torch.float32 or images.dim() != 4 or tuple(images.shape[2:]) != (self.plan.H, self.plan.W):
            raise RuntimeError(f"SpectrumStats.update: images must be f32 [b, C, {self.plan.H}, {self.plan.W}], got "
                               f"{images.dtype} {tuple(images.shape)}")
        if images.shape[0] == 0:
            return self
        ops.spectrum_accum(ops.spectrum_profiles(images.contiguous(), self.plan, self.center), self.sum, self.sumsq)
        self.n += int(images.shape[0])
        return self

    def merge(self, other: "SpectrumStats") -> "SpectrumStats":
        """Add another stream's sums (another rank's, another shard's): the statistics are additive."""
        if not self.plan.same_bins(other.plan) or self.center != other.center:
            raise RuntimeError(f"SpectrumStats.merge: the plans differ ({self.plan} vs {other.plan})")
        self.sum += other.sum.to(self.sum.device)
        self.sumsq += other.sumsq.to(self.sumsq.device)
        self.n += other.n
        return self

    def mean_profile(self) -> np.ndarray:
        """sum / n as a host f64 array [n_bins] (one copy of n_bins doubles)."""
        if self.n < 1:
            raise RuntimeError("SpectrumStats.mean_profile: no image yet")
        return self.sum.cpu().numpy() / self.n

    def var_profile(self) -> np.ndarray:
        """(sumsq - n mean^2) / (n - 1): the sample variance of the per-image profiles, a host f64 array [n_bins]."""
        if self.n < 2:
            raise RuntimeError("SpectrumStats.var_profile needs at least two images")
        m = self.sum.cpu().numpy() / self.n
        return (self.sumsq.cpu().numpy() - self.n * m * m) / (self.n - 1)

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return {"sum": self.sum, "sumsq": self.sumsq, "n": torch.tensor(self.n, dtype=torch.int64)}

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> "SpectrumStats":
        s, q = sd["sum"], sd["sumsq"]
        nb = self.plan.n_bins
        if s.dtype != torch.float64 or q.dtype != torch.float64 or tuple(s.shape) != (nb,) or tuple(q.shape) != (nb,):
            raise RuntimeError(f"SpectrumStats: sum and sumsq must be f64 [{nb}]")
        dev = self.sum.device
        self.sum, self.sumsq, self.n = s.to(dev).contiguous().clone(), q.to(dev).contiguous().clone(), int(sd["n"])
        return self


def _spectral_distance(plan, mean_real: np.ndarray, mean_fake: np.ndarray, skip_bins: int, hf_from: float) -> Dict[str, object]:
    """``spectral_distance`` on two host mean profiles."""
    k = np.arange(plan.n_bins)
    live = (k >= skip_bins) & (plan.counts > 0)
    both = live & (mean_real > 0) & (mean_fake > 0)
    d = 10.0 * np.log10(mean_real[both] / mean_fake[both])
    lsd = float(np.sqrt(np.mean(d * d))) if d.size else float("nan")
    hf = live & (plan.frac_lo >= hf_from)
    share = []
    for m in (mean_real, mean_fake):
        tot = float(m[live].sum())
        share.append(float(m[hf].sum()) / tot if tot > 0 else float("nan"))
    excess = 10.0 * math.log10(share[1] / share[0]) if share[0] > 0 and share[1] > 0 else float("nan")
    return {"lsd_db": lsd, "hf_share_real": share[0], "hf_share_fake": share[1], "hf_excess_db": excess,
            "bins_used": int(both.sum()), "bins_skipped": int(live.sum() - both.sum()), "mean_real": mean_real,
            "mean_fake": mean_fake, "centers": plan.centers.copy()}


def spectral_distance(real: SpectrumStats, fake: SpectrumStats, skip_bins: int = 1, hf_from: float = 0.5) -> Dict[str, object]:
    """Two image sets compared by their mean binned power spectra (host numpy f64 on 2 n_bins doubles):

        lsd_db         the log-spectral distance: the RMS of 10 log10(mean_real[k] / mean_fake[k]) over the bins k >= skip_bins
                       that hold at least one frequency (skip_bins = 1 leaves the lowest bin, DC and its leakage, out)
        hf_share_real  the share of the power of the bins k >= skip_bins that lies in bins whose lower edge is at or above
        hf_share_fake  hf_from of r_max (the Nyquist corner, sqrt(1/2) cycles per pixel)
        hf_excess_db   10 log10(hf_share_fake / hf_share_real): > 0, the generator puts too much into the top of the band

    plus mean_real, mean_fake, centers (cycles per pixel), bins_used and bins_skipped: a bin where either mean is 0 has no
    log ratio; it is left out of lsd_db and counted.  lsd_db is symmetric in its arguments, hf_excess_db changes sign."""
    if not isinstance(real, SpectrumStats) or not isinstance(fake, SpectrumStats):
        raise RuntimeError("spectral_distance: real and fake must be SpectrumStats")
    if not real.plan.same_bins(fake.plan) or real.center != fake.center:
        raise RuntimeError(f"spectral_distance: the plans differ ({real.plan} vs {fake.plan})")
    if isinstance(skip_bins, bool) or not isinstance(skip_bins, int) or not 0 <= skip_bins < real.plan.n_bins:
        raise RuntimeError(f"spectral_distance: skip_bins must be an integer in [0, n_bins = {real.plan.n_bins}), got {skip_bins!r}")
    hf_from = float(hf_from)
    if not 0.0 <= hf_from <= 1.0:
        raise RuntimeError(f"spectral_distance: hf_from is a fraction of r_max in [0, 1], got {hf_from}")
    if real.n < 1 or fake.n < 1:
        raise RuntimeError("spectral_distance needs at least one image on each side")
    return _spectral_distance(real.plan, real.mean_profile(), fake.mean_profile(), skip_bins, hf_from)


def _pr_counts(real_feats: torch.Tensor, fake_feats: torch.Tensor, k: int) -> torch.Tensor:
    """int64 [2] on the device: (fake rows inside the real manifold, real rows inside the fake manifold)."""
    _check_feats(real_feats, None, "precision_recall")
    _check_feats(fake_feats, real_feats.shape[1], "precision_recall")
    counts = torch.empty(2, dtype=torch.int64, device=real_feats.device)
    r2_real = ops.knn_radius2(real_feats, k)
    r2_fake = ops.knn_radius2(fake_feats, k)
    ops.manifold_cover(fake_feats, real_feats, r2_real, count=counts[0:1])
    ops.manifold_cover(real_feats, fake_feats, r2_fake, count=counts[1:2])
    return counts


def _pr_result(fake_in_real: int, real_in_fake: int, n_real: int, n_fake: int, k: int) -> Dict[str, float]:
    p, r = fake_in_real / n_fake, real_in_fake / n_real
    return {"precision": p, "recall": r, "f1": 0.0 if p + r == 0 else 2.0 * p * r / (p + r),
            "n_real": n_real, "n_fake": n_fake, "k": k}


def precision_recall(real_feats: torch.Tensor, fake_feats: torch.Tensor, k: int = 3) -> Dict[str, float]:
    """Improved precision and recall (Kynkaanniemi et al. 2019): the manifold of a set is the union of the balls around
    its samples that reach to each sample's k-th nearest neighbour in the set.
        precision = share of fake rows inside the real manifold,  recall = share of real rows inside the fake manifold,
        f1 = their harmonic mean (0 when both are 0);  plus n_real, n_fake, k.
    real_feats f32 [Nr, D], fake_feats f32 [Nf, D] on the device, k < min(Nr, Nf), k <= 8.  Distances in exact f32 on the
    MFMA (include/vaegan_hip.h states the form and its error bound); no N x N matrix is ever allocated.  Single process;
    ONE host sync at the end (two integers)."""
    k = int(k)
    c = _pr_counts(real_feats, fake_feats, k).tolist()                                 # the one host sync
    return _pr_result(c[0], c[1], real_feats.shape[0], fake_feats.shape[0], k)


def kid_subsets(Nr: int, Nf: int, subsets: int, subset_size: int, seed: int = 0):
    """The subset tables of ``kernel_distance``, drawn on the host: -> (idx_real, idx_fake), int32 numpy [subsets,
    subset_size].  One ``numpy.random.Generator(numpy.random.PCG64(seed))``; for each subset in turn
    ``permutation(Nr)[:m]`` first, then ``permutation(Nf)[:m]``: rows without repetition, as torchmetrics draws them."""
    Nr, Nf, S, m = int(Nr), int(Nf), int(subsets), int(subset_size)
    if S < 1 or m < 2:
        raise ValueError(f"kid_subsets: need subsets >= 1 and subset_size >= 2, got {S} and {m}")
    if m > min(Nr, Nf):
        raise ValueError(f"kid_subsets: subset_size {m} exceeds the smaller feature set ({min(Nr, Nf)} rows)")
    g = np.random.Generator(np.random.PCG64(int(seed)))
    ir, jf = np.empty((S, m), np.int32), np.empty((S, m), np.int32)
    for s in range(S):
        ir[s] = g.permutation(Nr)[:m]
        jf[s] = g.permutation(Nf)[:m]
    return ir, jf


def _check_table(t, S: int, m: int, N: int, name: str) -> np.ndarray:
    """An injected subset table on the host: integer [S, m] with every entry in [0, N) -> int32 numpy."""
    if isinstance(t, torch.Tensor):
        t = t.cpu().numpy()
    t = np.asarray(t)
    if t.ndim != 2 or t.shape != (S, m) or not np.issubdtype(t.dtype, np.integer):
        raise ValueError(f"kernel_distance: {name} must be an integer [{S}, {m}] table, got {t.dtype} {t.shape}")
    lo, hi = int(t.min()), int(t.max())
    if lo < 0 or hi >= N:
        raise ValueError(f"kernel_distance: {name} holds row indices in [{lo}, {hi}], the set has {N} rows")
    return np.ascontiguousarray(t, dtype=np.int32)


def _kid_device(real_feats, fake_feats, subsets, subset_size, degree, gamma, coef, seed, idx_real, idx_fake):
    """-> (scores f64 [S] and stat f64 [2] on the device, S, m, D); no host sync unless an injected table lives on the
    device (the tables are made or checked on the host)."""
    _check_feats(real_feats, None, "kernel_distance")
    _check_feats(fake_feats, real_feats.shape[1], "kernel_distance")
    Nr, Nf, D = int(real_feats.shape[0]), int(fake_feats.shape[0]), int(real_feats.shape[1])
    if (idx_real is None) != (idx_fake is None):
        raise ValueError("kernel_distance: give both idx_real and idx_fake, or neither")
    if idx_real is not None:
        shape = tuple(idx_real.shape)
        S, m = (int(shape[0]), int(shape[1])) if len(shape) == 2 else (int(subsets), int(subset_size))
    else:
        S, m = int(subsets), int(subset_size)
    if m > min(Nr, Nf):
        raise ValueError(f"kernel_distance: subset_size {m} exceeds the smaller feature set ({min(Nr, Nf)} rows)")
    if not (1 <= S <= 4096 and 2 <= m <= 32768):
        raise ValueError(f"kernel_distance: need 1 <= subsets <= 4096 and 2 <= subset_size <= 32768, got {S} and {m}")
    if idx_real is None:
        ir, jf = kid_subsets(Nr, Nf, S, m, seed)
    else:
        ir, jf = _check_table(idx_real, S, m, Nr, "idx_real"), _check_table(idx_fake, S, m, Nf, "idx_fake")
    dev = real_feats.device
    g = 1.0 / D if gamma is None else float(gamma)
    scores, stat, _ = ops.kid_scores(real_feats, fake_feats, torch.from_numpy(ir).to(dev), torch.from_numpy(jf).to(dev),
                                     int(degree), g, float(coef))
    return scores, stat, S, m, D


def kernel_distance(real_feats: torch.Tensor, fake_feats: torch.Tensor, subsets: int = 100, subset_size: int = 1000,
                    degree: int = 3, gamma: Optional[float] = None, coef: float = 1.0, seed: int = 0, idx_real=None,
                    idx_fake=None, return_scores: bool = False):
    """Kernel Inception Distance (Binkowski et al. 2018): for each of ``subsets`` random subset pairs of ``subset_size``
    rows, the unbiased MMD^2 estimate under k(a, c) = (gamma a.c + coef)^degree (``gamma=None``: 1 / D),

        score = (sum_{i != j} k(x_i, x_j) + sum_{i != j} k(y_i, y_j)) / (m (m - 1)) - 2 sum_{i, j} k(x_i, y_j) / m^2

    -> {"kid_mean", "kid_std" (POPULATION standard deviation over the subsets), "subsets", "subset_size",
    "feature_dim"}; with ``return_scores=True`` -> (that dict, the f64 [subsets] scores on the device).
    real_feats f32 [Nr, D], fake_feats f32 [Nf, D] on the device; ``subset_size > min(Nr, Nf)`` is a ValueError.
    The subsets are drawn on the host (``kid_subsets(Nr, Nf, subsets, subset_size, seed)``) and uploaded once as int32;
    ``idx_real`` / ``idx_fake`` inject tables instead (integer [S, m], numpy or torch; checked on the host for shape, dtype
    and range, which is a sync if they live on the device).  All arithmetic in f64 on the f64 MFMA, deterministic
    (include/vaegan_hip.h, vg_kid_scores); the m x m Gram matrix is never written.  Single process; ONE host sync at the
    end (two doubles).  The reference computes no KID; parity with torchmetrics is unpinned (not installed)."""
    scores, stat, S, m, D = _kid_device(real_feats, fake_feats, subsets, subset_size, degree, gamma, coef, seed, idx_real,
                                        idx_fake)
    mean, std = stat.tolist()                                                          # the one host sync
    out = {"kid_mean": mean, "kid_std": std, "subsets": S, "subset_size": m, "feature_dim": D}
    return (out, scores) if return_scores else out


def ndb_statistics(count_real, count_fake, alpha: float = 0.05) -> Dict[str, object]:
    """The host arithmetic of ``ndb`` on two K-length bin histograms (integer counts), numpy f64.  Per bin, with n, m the
    sample counts and P, Q the proportions: pooled p = (n P + m Q) / (n + m), se = sqrt(p (1 - p) (1 / n + 1 / m)),
    z = (P - Q) / se (0 where se = 0), two-sided p-value erfc(|z| / sqrt(2)); the bin is statistically different where
    p-value < alpha.  js_divergence = 0.5 KL(P || M) + 0.5 KL(Q || M), M = (P + Q) / 2, natural log, 0 log 0 = 0.
    -> ndb, ndb_over_k, js_divergence, bins (bool [K]), p_values, z, real_proportions, fake_proportions, n_real, n_fake."""
    cr, cf = np.asarray(count_real, dtype=np.float64), np.asarray(count_fake, dtype=np.float64)
    if cr.ndim != 1 or cr.shape != cf.shape or cr.size < 1:
        raise ValueError("ndb_statistics: two histograms of the same length K >= 1")
    n, m = cr.sum(), cf.sum()
    if n < 1 or m < 1:
        raise ValueError("ndb_statistics: both histograms need at least one sample")
    P, Q = cr / n, cf / m
    pooled = (n * P + m * Q) / (n + m)
    se = np.sqrt(pooled * (1.0 - pooled) * (1.0 / n + 1.0 / m))
    z = np.zeros_like(P)
    np.divide(P - Q, se, out=z, where=se > 0)
    pv = np.array([math.erfc(abs(v) / math.sqrt(2.0)) for v in z])
    bins = pv < float(alpha)
    M = 0.5 * (P + Q)

    def kl(a):
        nz = a > 0
        return float(np.sum(a[nz] * np.log(a[nz] / M[nz])))

    return {"ndb": int(bins.sum()), "ndb_over_k": float(bins.sum()) / P.size, "js_divergence": 0.5 * kl(P) + 0.5 * kl(Q),
            "bins": bins, "p_values": pv, "z": z, "real_proportions": P, "fake_proportions": Q, "n_real": int(n),
            "n_fake": int(m)}


def _ndb_device(real_feats, fake_feats, n_bins, seed, kmeans):
    """-> (the KMeans of the real rows, int64 [2, K] on the device: real and fake bin counts)."""
    _check_feats(fake_feats, None, "ndb")
    if kmeans is None:
        _check_feats(real_feats, fake_feats.shape[1], "ndb")
        kmeans = KMeans.fit(real_feats, int(n_bins), seed=int(seed))
    elif not isinstance(kmeans, KMeans) or kmeans.dim != fake_feats.shape[1]:
        raise RuntimeError(f"ndb: kmeans must be a fitted cluster.KMeans over {fake_feats.shape[1]}-dimensional rows")
    if fake_feats.shape[0] < 1:
        raise RuntimeError("ndb: fake_feats must hold at least one row")
    fake_count = ops.kmeans_update(fake_feats, kmeans.predict(fake_feats), kmeans.n_clusters)[0]
    return kmeans, torch.stack([kmeans.counts_, fake_count])


def ndb(real_feats: Optional[torch.Tensor], fake_feats: torch.Tensor, n_bins: int = 100, alpha: float = 0.05, seed: int = 0,
        kmeans: Optional[KMeans] = None) -> Dict[str, object]:
    """Number of statistically Different Bins (Richardson & Weiss 2018, "On GANs and GMMs"): k-means clusters the REAL
    features into ``n_bins`` bins (``cluster.KMeans.fit``, k-means++ from ``seed``), every fake row goes to its nearest
    centre, and a two-proportion z-test per bin counts the bins whose shares differ at level ``alpha``
    (``ndb_statistics``).  It needs no classifier and says WHICH modes a Generator dropped: ``bins`` marks them.
    real_feats f32 [Nr, D], fake_feats f32 [Nf, D] on the device.  kmeans: a ``KMeans`` of the real side fitted earlier
    (returned by every call as ``kmeans``) -- cluster the real features once per training run; real_feats may then be None
    and n_bins / seed are not read.  -> the keys of ``ndb_statistics`` plus ``kmeans``.  Besides the fit (one host sync per
    Lloyd iteration): two launches for the fake side and one host sync of 2 K integers.  No feature whitening; single
    process, like precision / recall."""
    kmeans, counts = _ndb_device(real_feats, fake_feats, n_bins, seed, kmeans)
    c = counts.cpu().numpy()                                                           # the one host sync
    out = ndb_statistics(c[0], c[1], alpha)
    out["kmeans"] = kmeans
    return out


_ARANGE = {}


def _arange(n: int, device) -> torch.Tensor:
    key = (n, str(device))
    t = _ARANGE.get(key)
    if t is None:
        t = _ARANGE[key] = torch.arange(n, dtype=torch.int64, device=device)
    return t


def encoder_features(encoder, part: str = "mu") -> Callable[[torch.Tensor], torch.Tensor]:
    """-> ``feature_fn(images_u8) -> f32 [b, L]`` (``part="mu"``) or ``[b, 2L]`` (``part="mulv"``: mu | logvar): uint8
    [b,C,S,S] device images -> x / 255 * 2 - 1 (the data path's ToTensor + Normalize arithmetic, (u/255 - 0.5)/0.5) ->
    the eval-mode Encoder through the engine.  uint8 in, because that is what the reference hands to its metrics
    (vaegan_code.py:176-183) and what ``ops.to_u8`` produces.  The features are the project's own: an FID in this space
    is comparable between checkpoints scored with the SAME encoder, not with published Inception FIDs."""
    if part not in ("mu", "mulv"):
        raise RuntimeError(f"encoder_features: part must be 'mu' or 'mulv', got {part!r}")
    width = encoder.latent_dim * (1 if part == "mu" else 2)

    @torch.no_grad()
    def feature_fn(images_u8: torch.Tensor) -> torch.Tensor:
        if not images_u8.is_cuda:
            raise RuntimeError("encoder_features needs device images ('cuda'); there is no CPU path")
        if images_u8.dtype != torch.uint8 or images_u8.dim() != 4:
            raise RuntimeError("encoder_features: images must be uint8 [b,C,S,S]")
        encoder.eval()
        b, C, H, W = images_u8.shape
        planes = images_u8.contiguous().view(b * C, H, W, 1)               # every channel plane as a 1-channel image
        x = ops.gather_normalize_u8(planes, _arange(b * C, images_u8.device)).view(b, C, H, W)
        mulv, _ = encoder.engine_forward(x, keep=False)
        out = torch.empty(b, width, dtype=torch.float32, device=images_u8.device)
        out.copy_(mulv[:, :width])                                          # widening copy of the real columns
        return out

    return feature_fn


class FeaturePass:
    """What an evaluation loop keeps while it runs with a ``feature_fn``: per-batch FID statistics of both sides and,
    with ``keep=True``, the features themselves (on the device) for precision / recall at the end of the pass."""

    def __init__(self, feature_fn, keep: bool, real_stats: Optional[FeatureStats] = None):
        self.fn, self.keep, self.given_real = feature_fn, keep, real_stats
        self.real, self.fake = real_stats, None
        self.real_feats, self.fake_feats = [], []
        self.D = real_stats.D if real_stats is not None else None

    def _features(self, img: torch.Tensor) -> torch.Tensor:
        f = self.fn(ops.to_u8(img))
        _check_feats(f, self.D, "feature_fn")
        if f.shape[0] != img.shape[0]:
            raise RuntimeError(f"feature_fn returned {f.shape[0]} rows for {img.shape[0]} images")
        if self.D is None:
            self.D = int(f.shape[1])
        return f.contiguous()

    def update(self, real: torch.Tensor, fake: torch.Tensor) -> None:
        """real, fake: f32 [b,C,S,S] device images in [-1, 1]."""
        need_real = self.given_real is None or self.keep
        fr = self._features(real) if need_real else None
        ff = self._features(fake)
        if self.fake is None:
            self.fake = FeatureStats(self.D, ff.device)
            if self.real is None:
                self.real = FeatureStats(self.D, ff.device)
        if self.given_real is None:
            self.real.update(fr)
        self.fake.update(ff)
        if self.keep:
            self.real_feats.append(fr)
            self.fake_feats.append(ff)

    def pr_counts(self, k: int) -> torch.Tensor:
        return _pr_counts(torch.cat(self.real_feats), torch.cat(self.fake_feats), k)

    def fid(self) -> float:
        return frechet_distance(self.real, self.fake)

    def kid(self, subsets: int, subset_size: int = 1000, seed: int = 0) -> torch.Tensor:
        """f64 [2] on the device: mean and population standard deviation of the pass's KID scores (``keep=True``)."""
        if not self.keep:
            raise RuntimeError("FeaturePass.kid needs the features of the pass: construct it with keep=True")
        return _kid_device(torch.cat(self.real_feats), torch.cat(self.fake_feats), subsets, subset_size, 3, None, 1.0, seed,
                           None, None)[1]

    def ndb_counts(self, n_bins: int, seed: int = 0) -> torch.Tensor:
        """int64 [2, n_bins] on the device: the real and fake bin counts of the pass's features (``keep=True``); the
        k-means fit inside costs one host sync per Lloyd iteration."""
        if not self.keep:
            raise RuntimeError("FeaturePass.ndb_counts needs the features of the pass: construct it with keep=True")
        return _ndb_device(torch.cat(self.real_feats), torch.cat(self.fake_feats), n_bins, seed, None)[1]
