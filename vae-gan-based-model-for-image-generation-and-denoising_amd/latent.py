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

Beyond the reference: ``GaussianMixturePrior`` fits a full-covariance Gaussian mixture to the same latents by EM on the
device (vg_gmm_log_resp, vg_gmm_moments; the K small D x D steps in numpy on the host) and samples it there
(vg_gmm_sample) -- the histogram prior treats every latent dimension on its own, the mixture keeps their correlations.
Either prior is a ``prior=`` of ``evaluate_generation`` / ``sample_images``.
"""
from typing import Dict, Iterable, Optional, Tuple, Union

import numpy as np
import torch

from . import geometry as G
from . import ops
from .cluster import KMeans
from . import spectrum as _spectrum
from .metrics import FeaturePass, SpectrumStats, _pr_result, _spectral_distance, ndb_statistics


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


_GMM_TINY = 10 * np.finfo(np.float64).eps
_GMM_KEYS = ("weights", "means", "covariances", "prec_chol", "cov_chol", "cdf")


def _lower_inverse(low: np.ndarray) -> np.ndarray:
    """Inverse of a lower-triangular matrix by forward substitution (exactly lower triangular, f64)."""
    D = low.shape[0]
    inv = np.zeros_like(low)
    for i in range(D):
        row = -(low[i, :i] @ inv[:i])
        row[i] += 1.0
        inv[i] = row / low[i, i]
    return inv


def _gmm_host_step(weights: np.ndarray, means: np.ndarray, cov: np.ndarray, reg_covar: float) -> Dict[str, np.ndarray]:
    """The K small D x D steps of an M-step, numpy f64 on the host: Cholesky factor L_k of every covariance, the
    precision factor U_k = inverse(L_k)^T (scikit-learn's precisions_cholesky_), log_coef and the cdf of the weights."""
    K, D = means.shape
    cov_chol, prec_chol = np.empty_like(cov), np.empty_like(cov)
    for k in range(K):
        try:
            if not np.all(np.isfinite(cov[k])):
                raise np.linalg.LinAlgError("not finite")
            cov_chol[k] = np.linalg.cholesky(cov[k])
        except np.linalg.LinAlgError:
            raise RuntimeError(f"GaussianMixturePrior.fit: the covariance of component {k} is not positive definite "
                               f"(a collapsed component or a degenerate latent column); increase reg_covar "
                               f"(now {reg_covar})") from None
        prec_chol[k] = _lower_inverse(cov_chol[k]).T
    log_det = np.log(np.diagonal(prec_chol, axis1=1, axis2=2)).sum(axis=1)
    log_coef = np.log(weights) + log_det - 0.5 * D * np.log(2.0 * np.pi)
    return dict(weights=weights, means=means, covariances=cov, cov_chol=cov_chol, prec_chol=prec_chol, log_coef=log_coef,
                cdf=np.cumsum(weights))


class GaussianMixturePrior:
    """A full-covariance Gaussian mixture fitted to the aggregate posterior (ex-post density estimation, Ghosh et al.
    2020); not in the reference, whose histogram prior (``LatentPrior``) fits every latent dimension on its own and so
    discards the correlations between them.  The two GEMM-shaped phases of EM and the sampler are HIP kernels
    (include/vaegan_hip.h, "Gaussian-mixture prior"); the latents never leave the device.

    Device tensors, all f64: ``weights`` [K], ``means`` [K, D], ``covariances`` [K, D, D], ``prec_chol`` [K, D, D] (upper
    factors U_k, inverse(Sigma_k) = U_k U_k^T: scikit-learn's precisions_cholesky_), ``cov_chol`` [K, D, D] (lower factors
    L_k of Sigma_k), ``cdf`` [K] (np.cumsum(weights)).  Python values: ``converged``, ``n_iter``, ``lower_bound`` (the mean
    log-likelihood per row of the last E-step), ``n_fitted``, ``latent_dim``."""

    def __init__(self, weights, means, covariances, prec_chol, cov_chol, cdf, converged: bool = True, n_iter: int = 0,
                 lower_bound: float = float("nan"), n_fitted: int = 0):
        ts = (weights, means, covariances, prec_chol, cov_chol, cdf)
        for t in ts:
            if not t.is_cuda:
                raise RuntimeError("GaussianMixturePrior lives on the MI355X ('cuda'); there is no CPU path")
        K, D = (means.shape[0], means.shape[1]) if means.dim() == 2 else (0, 0)
        shapes = ((K,), (K, D), (K, D, D), (K, D, D), (K, D, D), (K,))
        if K < 1 or D < 1 or any(t.dtype != torch.float64 or tuple(t.shape) != s for t, s in zip(ts, shapes)):
            raise RuntimeError("GaussianMixturePrior: f64 weights [K], means [K,D], covariances / prec_chol / cov_chol "
                               "[K,D,D], cdf [K]")
        self.weights, self.means, self.covariances, self.prec_chol, self.cov_chol, self.cdf = (t.contiguous() for t in ts)
        self.n_components, self.latent_dim = K, D
        self.converged, self.n_iter = bool(converged), int(n_iter)
        self.lower_bound, self.n_fitted = float(lower_bound), int(n_fitted)
        self._log_coef = None                                           # f64 [K] on the device, made on first use

    @classmethod
    def fit(cls, x: torch.Tensor, n_components: int = 10, reg_covar: float = 1e-6, tol: float = 1e-3, max_iter: int = 100,
            seed: int = 0, init_idx=None, init="random") -> "GaussianMixturePrior":
        """EM on x f32 [N, D] on the device, possibly a strided view: fit on the ``mu`` columns of ``encode_dataset``'s
        output, ``mulv[:, :L]`` (no copy is made).  Fitting on sampled z instead is out of scope.

        Initialisation: ``init_idx`` (K distinct row numbers; default ``np.random.default_rng(seed).choice(N, K,
        replace=False)``) names the rows that become the means; weights 1 / K; every precision diag(1 / (var + reg_covar))
        with var the global per-column variance (one ``ops.gmm_moments`` call with K = 1, resp = 1).  That is
        ``init="random"``, the default.  ``init="kmeans"`` (a ``cluster.KMeans`` fitted here by k-means++ from ``seed``) or
        ``init=<a fitted KMeans>`` of the same K and D is scikit-learn's default ``init_params="kmeans"``: one
        ``ops.kmeans_assign`` gives the one-hot responsibilities, ``ops.gmm_moments`` around the centres their sums, and the
        host M-step of the loop below the starting weights, means and covariances (``_initialize_parameters`` followed by
        ``_initialize``); from there EM needs fewer iterations and ends in better optima.  ``init_idx`` belongs to
        ``init="random"`` and is refused with a k-means start; so is a start that leaves a cluster empty.
        Loop: exactly scikit-learn's ``GaussianMixture.fit`` -- E-step (``ops.gmm_log_resp``), lower_bound = mean
        log-likelihood, M-step (``ops.gmm_moments`` around the current means, then the K small D x D steps in numpy f64 on
        the host: weights, means, Sigma_k + reg_covar I, Cholesky, triangular inverse, log_coef, cdf -- the precedent of
        ``metrics.frechet_distance``), stop when |change of lower_bound| < tol; nk gets + 10 eps.  Three launches and ONE
        host sync per iteration.  Not converged after max_iter: ``converged`` is False, no warning.
        RuntimeError: N < K, a bad init_idx, a failed Cholesky or a non-finite lower_bound (a NaN latent, a constant
        column with reg_covar = 0): the message names reg_covar."""
        if not x.is_cuda:
            raise RuntimeError("GaussianMixturePrior.fit needs the latents on the MI355X ('cuda'); there is no CPU path")
        if x.dim() != 2 or x.dtype != torch.float32:
            raise RuntimeError("GaussianMixturePrior.fit: x must be f32 [N, D]")
        N, D = x.shape
        K = int(n_components)
        if not (1 <= K <= ops.GMM_MAX_K and 1 <= D <= ops.GMM_MAX_D):
            raise RuntimeError(f"GaussianMixturePrior.fit: needs 1 <= n_components <= {ops.GMM_MAX_K} and 1 <= D <= "
                               f"{ops.GMM_MAX_D}")
        if N < K:
            raise RuntimeError(f"GaussianMixturePrior.fit: {N} rows cannot initialise {K} components (reg_covar does not "
                               f"help here: give more rows or fewer components)")
        kmeans_start = not (isinstance(init, str) and init == "random")
        if kmeans_start:
            if not (isinstance(init, KMeans) or (isinstance(init, str) and init == "kmeans")):
                raise RuntimeError(f"GaussianMixturePrior.fit: init must be 'random', 'kmeans' or a fitted KMeans, got "
                                   f"{init!r}")
            if init_idx is not None:
                raise RuntimeError("GaussianMixturePrior.fit: init_idx names the rows of init='random'; a k-means start "
                                   "takes its centres from the clustering")
            if isinstance(init, KMeans) and (init.n_clusters, init.dim) != (K, D):
                raise RuntimeError(f"GaussianMixturePrior.fit: the KMeans has {init.n_clusters} clusters of {init.dim} "
                                   f"dimensions, the mixture {K} components of {D}")
        else:
            if init_idx is None:
                init_idx = np.random.default_rng(seed).choice(N, K, replace=False)
            idx = np.asarray(init_idx)
            if (idx.ndim != 1 or idx.size != K or not np.issubdtype(idx.dtype, np.integer) or idx.min() < 0
                    or idx.max() >= N or np.unique(idx).size != K):
                raise RuntimeError(f"GaussianMixturePrior.fit: init_idx must be {K} distinct row numbers in [0, {N})")
        if max_iter < 1:
            raise RuntimeError("GaussianMixturePrior.fit: max_iter must be >= 1")
        dev = x.device
        up = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(dev)      # noqa: E731

        def m_step(nk_raw, s1_h, s2_h, means):
            nk_h = nk_raw + _GMM_TINY
            weights = nk_h / N
            weights = weights / weights.sum()
            delta = s1_h / nk_h[:, None]
            means = means + delta
            cov = s2_h / nk_h[:, None, None] - delta[:, :, None] * delta[:, None, :]
            cov = 0.5 * (cov + cov.transpose(0, 2, 1))
            cov[:, np.arange(D), np.arange(D)] += reg_covar
            return _gmm_host_step(weights, means, cov, reg_covar)

        if kmeans_start:
            return cls._fit_loop(x, K, reg_covar, tol, max_iter, m_step, up,
                                 *cls._kmeans_start(x, K, seed, init, m_step, up))
        rows = x[torch.as_tensor(idx, dtype=torch.int64, device=dev)].double().contiguous()      # [K, D]
        nk, s1, s2, _ = ops.gmm_moments(x, rows[:1].contiguous(), torch.ones(N, 1, dtype=torch.float64, device=dev))
        nk0 = float(nk.item())
        delta = s1[0].cpu().numpy() / nk0
        var = np.diagonal(s2[0].cpu().numpy()) / nk0 - delta * delta
        with np.errstate(divide="ignore", invalid="ignore"):
            prec = 1.0 / (var + reg_covar)
        if not np.all(np.isfinite(prec)) or np.any(prec <= 0.0):
            raise RuntimeError(f"GaussianMixturePrior.fit: a latent column has no finite positive variance (a NaN, an "
                               f"infinity or a constant column); increase reg_covar (now {reg_covar})")
        weights = np.full(K, 1.0 / K)
        means = rows.cpu().numpy()
        log_coef = np.log(weights) + np.log(np.sqrt(prec)).sum() - 0.5 * D * np.log(2.0 * np.pi)
        d_means, d_prec, d_coef = rows, up(np.tile(np.diag(np.sqrt(prec)), (K, 1, 1))), up(log_coef)
        return cls._fit_loop(x, K, reg_covar, tol, max_iter, m_step, up, means, d_means, d_prec, d_coef)

    @staticmethod
    def _kmeans_start(x, K, seed, init, m_step, up):
        """scikit-learn's init_params="kmeans": -> (means, d_means, d_prec, d_coef) of the M-step on one-hot
        responsibilities."""
        N = x.shape[0]
        km = init if isinstance(init, KMeans) else KMeans.fit(x, K, seed=seed)
        centres = km.cluster_centers_
        _, _, resp, _ = ops.kmeans_assign(x, centres, want_label=False, want_resp=True)
        nk, s1, s2, _ = ops.gmm_moments(x, centres, resp)
        D = centres.shape[1]
        flat = torch.cat([nk, s1.reshape(-1), s2.reshape(-1), centres.reshape(-1)]).cpu().numpy()
        nk_h = flat[:K]
        if np.any(nk_h == 0.0):
            raise RuntimeError(f"GaussianMixturePrior.fit: the k-means start leaves cluster {int(np.argmin(nk_h))} of {K} "
                               f"empty ({N} rows); ask for fewer components or use init='random'")
        p = m_step(nk_h, flat[K:K + K * D].reshape(K, D), flat[K + K * D:K + K * D + K * D * D].reshape(K, D, D),
                   flat[K + K * D + K * D * D:].reshape(K, D))
        return p["means"], up(p["means"]), up(p["prec_chol"]), up(p["log_coef"])

    @classmethod
    def _fit_loop(cls, x, K, reg_covar, tol, max_iter, m_step, up, means, d_means, d_prec, d_coef):
        """The EM loop of ``fit`` from a start: host means f64 [K, D] and their device twins."""
        N, D = x.shape
        lower, converged, n_iter, p = -np.inf, False, 0, None
        for n_iter in range(1, int(max_iter) + 1):
            prev = lower
            _, ln, resp = ops.gmm_log_resp(x, d_means, d_prec, d_coef)
            nk, s1, s2, ll = ops.gmm_moments(x, d_means, resp, ln)
            flat = torch.cat([ll, nk, s1.reshape(-1), s2.reshape(-1)]).cpu().numpy()               # the one host sync
            lower = float(flat[0]) / N
            if not np.isfinite(lower):
                raise RuntimeError(f"GaussianMixturePrior.fit: the log-likelihood is not finite in iteration {n_iter} (a "
                                   f"NaN or infinite latent, or a collapsed component); check the latents or increase "
                                   f"reg_covar (now {reg_covar})")
            p = m_step(flat[1:1 + K], flat[1 + K:1 + K + K * D].reshape(K, D), flat[1 + K + K * D:].reshape(K, D, D), means)
            means = p["means"]
            d_means, d_prec, d_coef = up(p["means"]), up(p["prec_chol"]), up(p["log_coef"])
            if abs(lower - prev) < tol:
                converged = True
                break
        out = cls(*(up(p[k]) for k in _GMM_KEYS), converged=converged, n_iter=n_iter, lower_bound=lower, n_fitted=N)
        out._log_coef = d_coef
        return out

    def _state(self, need: bool):
        if not need:
            return None
        ns = ops.default_noise(self.means.device)
        ns.advance()
        return ns.state

    def sample(self, n: int, u: Optional[torch.Tensor] = None, eps: Optional[torch.Tensor] = None) -> torch.Tensor:
        """n draws -> f32 [n, D].  u f64 [n] picks the component (np.searchsorted(cdf, u, side="right")), eps f32 [n, D] is
        the normal draw of z = mean_k + L_k eps; by default both come from the device stream, which advances by one step
        per call."""
        _, z32, _ = ops.gmm_sample(self.cdf, self.means, self.cov_chol, n, u, eps, self._state(u is None or eps is None))
        return z32

    def sample_z(self, n: int, dtype_of=None, u=None, eps=None, return_comp: bool = False):
        """n draws in ONE launch, in the input layout of the decoder ``dtype_of`` ([n, 1, 1, ZP] in its engine dtype, pad
        columns zero; f32 when dtype_of is None).  return_comp: -> (z, comp int32 [n])."""
        D = self.latent_dim
        dt = G.F32 if dtype_of is None else dtype_of._dt
        nz = D if dtype_of is None else dtype_of.nz
        if nz != D:
            raise RuntimeError(f"GaussianMixturePrior.sample_z: the decoder takes nz = {nz} inputs, the prior has {D} "
                               f"dimensions")
        comp, _, z = ops.gmm_sample(self.cdf, self.means, self.cov_chol, n, u, eps, self._state(u is None or eps is None),
                                    want_comp=return_comp, want_z32=False, z=(G.padc(nz, dt), dt))
        return (z, comp) if return_comp else z

    def score_samples(self, x: torch.Tensor) -> torch.Tensor:
        """log p(x) of every row of x f32 [N, D] (device) -> f64 [N]: the E-step's log_norm."""
        if x.dim() != 2 or x.shape[1] != self.latent_dim:
            raise RuntimeError(f"GaussianMixturePrior.score_samples: x must be [N, {self.latent_dim}]")
        if self._log_coef is None:                                      # a loaded prior: K values, once, on the host
            log_det = np.log(np.diagonal(self.prec_chol.cpu().numpy(), axis1=1, axis2=2)).sum(axis=1)
            coef = np.log(self.weights.cpu().numpy()) + log_det - 0.5 * self.latent_dim * np.log(2.0 * np.pi)
            self._log_coef = torch.as_tensor(coef, dtype=torch.float64).to(self.means.device)
        _, ln, _ = ops.gmm_log_resp(x, self.means, self.prec_chol, self._log_coef, want_resp=False)
        return ln

    def score(self, x: torch.Tensor) -> float:
        """Mean log-likelihood per row (scikit-learn's GaussianMixture.score); one host sync."""
        ln = self.score_samples(x)
        # The sum of the N values is vg_gmm_moments' loglik_sum -- f64, fixed order, the same bits on every call, what fit's
        # lower_bound is made of -- asked of ONE column with K = 1, so the moments that come with it cost next to nothing.
        col = x[:, :1]
        ones = torch.ones(x.shape[0], 1, dtype=torch.float64, device=x.device)
        ll = ops.gmm_moments(col, torch.zeros(1, 1, dtype=torch.float64, device=x.device), ones, ln)[3]
        return float(ll.item()) / x.shape[0]

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """Plain tensors: save a fitted prior beside the decoder checkpoint and sample without the data set."""
        sd = {k: getattr(self, k) for k in _GMM_KEYS}
        sd.update(converged=torch.tensor(self.converged), n_iter=torch.tensor(self.n_iter),
                  lower_bound=torch.tensor(self.lower_bound, dtype=torch.float64), n_fitted=torch.tensor(self.n_fitted))
        return sd

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> "GaussianMixturePrior":
        """Replace this prior's parameters by those of ``sd`` (a ``state_dict()``, e.g. from torch.load), moved to its device."""
        dev = self.means.device
        self.__init__(*(sd[k].to(dev) for k in _GMM_KEYS), converged=bool(sd["converged"]), n_iter=int(sd["n_iter"]),
                      lower_bound=float(sd["lower_bound"]), n_fitted=int(sd["n_fitted"]))
        return self

    @classmethod
    def from_state_dict(cls, sd: Dict[str, torch.Tensor], device="cuda") -> "GaussianMixturePrior":
        return cls(*(sd[k].to(device) for k in _GMM_KEYS), converged=bool(sd["converged"]), n_iter=int(sd["n_iter"]),
                   lower_bound=float(sd["lower_bound"]), n_fitted=int(sd["n_fitted"]))


def _device_of(decoder, what: str):
    dev = next(decoder.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError(f"{what} needs the decoder on the MI355X ('cuda'); there is no CPU path")
    return dev


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
def evaluate_generation(decoder, val_loader: Iterable[torch.Tensor],
                        prior: Optional[Union[LatentPrior, GaussianMixturePrior]] = None,
                        noise_fn=None, feature_fn=None, k: int = 3, real_stats=None, kid_subsets: Optional[int] = None,
                        kid_subset_size: int = 1000, kid_seed: int = 0) -> Dict[str, float]:
    """The generation-evaluation loops of the reference:

        decoder.eval()                                                                  (main_vae.py:476 / :546)
        for real in val_loader:   b = real.size(0)
            prior given  (:482-489): mu, logvar ~ histogram prior; z = mu + exp(logvar / 2) * randn; fake = G(z)
            mixture prior (a GaussianMixturePrior; not in the reference): z ~ the fitted mixture; fake = G(z)
            prior=None   (:552-554): z = randn(b, latent); fake = G(z)
            ssim.update((fake + 1) / 2, (real + 1) / 2)                                 (:492-496 / :557-561)
        ssim.compute()                                                   (mean over all images, ragged batch weighted)

    val_loader yields device batches [b,C,S,S] in [-1,1] (data.DeviceLoader).  noise_fn(i, b) injects the draws of batch
    i (parity tests): with a prior it returns (u, v, eps) -- f64 [b,2L], f64 [b,2L], f32 [b,L], see LatentPrior.sample_z --
    with a GaussianMixturePrior (u, eps) -- f64 [b], f32 [b,L], see GaussianMixturePrior.sample_z -- and without a prior
    the f32 [b, nz] z itself; by default everything is drawn on the device.  SSIM: torchmetrics recipe,
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
    deviation), read in the same host sync.  Not in the reference; single process, like precision / recall.

    NDB of the pass's features: ``evaluate_generation_ndb`` (this function's keyword list is pinned); the radial power
    spectra of the pass's images: ``evaluate_generation_spectrum``."""
    return _evaluate_generation(decoder, val_loader, prior, noise_fn, feature_fn, k, real_stats, kid_subsets,
                                kid_subset_size, kid_seed, None)


@torch.no_grad()
def evaluate_generation_ndb(decoder, val_loader: Iterable[torch.Tensor], ndb_bins: int = 100, ndb_alpha: float = 0.05,
                            ndb_seed: int = 0, **kwargs) -> Dict[str, float]:
    """``evaluate_generation(decoder, val_loader, **kwargs)`` whose result also holds ``ndb``, ``ndb_over_k`` and
    ``js_divergence`` (``metrics.ndb``: ``ndb_bins`` k-means bins of the pass's kept REAL features, k-means++ from
    ``ndb_seed``, two-proportion z-test at level ``ndb_alpha``).  Needs ``feature_fn=``, else RuntimeError, like
    ``kid_subsets``.  The k-means fit adds one host sync per Lloyd iteration to the pass; the bin counts are read in the
    pass's final sync.  Not in the reference; single process."""
    if kwargs.get("feature_fn") is None:
        raise RuntimeError("evaluate_generation_ndb: ndb_bins needs a feature_fn (NDB is a feature-space metric)")
    names = ("prior", "noise_fn", "feature_fn", "k", "real_stats", "kid_subsets", "kid_subset_size", "kid_seed")
    unknown = sorted(set(kwargs) - set(names))
    if unknown:
        raise TypeError(f"evaluate_generation_ndb: unknown keyword(s) {unknown}")
    defaults = dict(prior=None, noise_fn=None, feature_fn=None, k=3, real_stats=None, kid_subsets=None, kid_subset_size=1000,
                    kid_seed=0)
    defaults.update(kwargs)
    return _evaluate_generation(decoder, val_loader, *(defaults[n] for n in names),
                                (int(ndb_bins), float(ndb_alpha), int(ndb_seed)))


@torch.no_grad()
def evaluate_generation_spectrum(decoder, val_loader: Iterable[torch.Tensor], spectrum_bins: Optional[int] = None,
                                 window: str = "hann", **kwargs) -> Dict[str, float]:
    """``evaluate_generation(decoder, val_loader, **kwargs)`` whose result also holds ``lsd_db``, ``hf_excess_db``,
    ``hf_share_real`` and ``hf_share_fake`` (``metrics.spectral_distance`` with its defaults): the ``real`` and ``fake``
    images of every batch also go to two ``metrics.SpectrumStats`` over ``spectrum.spectrum_plan(H, W, spectrum_bins,
    window)`` -- radially binned power spectra on the device, no network and no feature_fn needed.  It is the one metric of
    the pass that sees the top octave, where stacks of ConvTranspose2d fail (Durall et al. 2020).  The 2 x 2 n_bins sums
    are read in the pass's final host sync; every other key is what ``evaluate_generation`` returns.  Not in the reference
    for images (it compares mean PSDs of EEG, test_eegglow.py:25-46)."""
    names = ("prior", "noise_fn", "feature_fn", "k", "real_stats", "kid_subsets", "kid_subset_size", "kid_seed")
    unknown = sorted(set(kwargs) - set(names))
    if unknown:
        raise TypeError(f"evaluate_generation_spectrum: unknown keyword(s) {unknown}")
    if window not in _spectrum.WINDOWS:
        raise RuntimeError(f"evaluate_generation_spectrum: window must be one of {_spectrum.WINDOWS}, got {window!r}")
    if spectrum_bins is not None and (isinstance(spectrum_bins, bool) or not isinstance(spectrum_bins, int) or spectrum_bins < 1):
        raise RuntimeError(f"evaluate_generation_spectrum: spectrum_bins must be a positive integer or None, got {spectrum_bins!r}")
    defaults = dict(prior=None, noise_fn=None, feature_fn=None, k=3, real_stats=None, kid_subsets=None, kid_subset_size=1000,
                    kid_seed=0)
    defaults.update(kwargs)
    return _evaluate_generation(decoder, val_loader, *(defaults[n] for n in names), None, (spectrum_bins, window))


def _evaluate_generation(decoder, val_loader, prior, noise_fn, feature_fn, k, real_stats, kid_subsets, kid_subset_size,
                         kid_seed, ndb, spectrum=None):
    """The pass behind ``evaluate_generation`` (ndb None), ``evaluate_generation_ndb`` (ndb = (bins, alpha, seed)) and
    ``evaluate_generation_spectrum`` (spectrum = (n_bins or None, window); default None: off)."""
    if kid_subsets is not None and feature_fn is None:
        raise RuntimeError("evaluate_generation: kid_subsets needs a feature_fn (KID is a feature-space metric)")
    decoder.eval()
    dev = _device_of(decoder, "evaluate_generation")
    acc = ops.zeros_f32(1, dev)
    seen = batches = 0
    feats = FeaturePass(feature_fn, True, real_stats) if feature_fn is not None else None
    spec = None
    for i, real in enumerate(val_loader):
        if not real.is_cuda:
            raise RuntimeError("evaluate_generation needs device batches (data.DeviceLoader); there is no CPU path")
        real = real.contiguous()
        b = real.shape[0]
        inj = noise_fn(i, b) if noise_fn is not None else None
        if isinstance(prior, GaussianMixturePrior):
            u, eps = inj if inj is not None else (None, None)
            z = prior.sample_z(b, decoder, u, eps)
        elif prior is not None:
            u, v, eps = inj if inj is not None else (None, None, None)
            z = prior.sample_z(b, decoder, u, v, eps)
        else:
            z = _normal_z(decoder, b, inj)
        fake = decoder.decode_eval(z, b)
        ops.axpy(acc, ops.ssim(fake, real), float(b), out=acc)
        if feats is not None:
            feats.update(real, fake)
        if spectrum is not None:
            if spec is None:
                plan = _spectrum.spectrum_plan(int(real.shape[2]), int(real.shape[3]), spectrum[0], spectrum[1])
                spec = (SpectrumStats(plan, dev), SpectrumStats(plan, dev))
            spec[0].update(real)
            spec[1].update(fake)
        seen += b
        batches += 1
    if batches == 0:
        raise RuntimeError("evaluate_generation: the loader yielded no batch")
    spec_parts = [spec[0].sum, spec[1].sum] if spec is not None else []
    if feats is None:
        if spec is None:
            return {"ssim": float(acc.item()) / seen, "samples": seen, "batches": batches}   # the one host sync
        ssim_sum, *sp = torch.cat([acc.double()] + spec_parts).tolist()                  # the one host sync
        out = {"ssim": ssim_sum / seen, "samples": seen, "batches": batches}
        out.update(_spectrum_result(spec, sp))
        return out
    counts = feats.pr_counts(int(k))
    parts = [acc.double(), counts.double()]
    if kid_subsets is not None:
        parts.append(feats.kid(int(kid_subsets), int(kid_subset_size), int(kid_seed)))
    if ndb is not None:
        parts.append(feats.ndb_counts(ndb[0], ndb[2]).double().reshape(-1))            # exact: counts are below 2^53
    parts += spec_parts
    ssim_sum, fake_in_real, real_in_fake, *kid = torch.cat(parts).tolist()             # the one host sync
    if spec is not None:
        sp = kid[len(kid) - 2 * spec[0].plan.n_bins:]
        kid = kid[:len(kid) - 2 * spec[0].plan.n_bins]
    if ndb is not None:
        bins = np.asarray(kid[len(kid) - 2 * ndb[0]:]).reshape(2, ndb[0])
        kid = kid[:len(kid) - 2 * ndb[0]]
    out = {"ssim": ssim_sum / seen, "samples": seen, "batches": batches, "fid": feats.fid(), "feature_dim": feats.D}
    pr = _pr_result(int(fake_in_real), int(real_in_fake), seen, seen, int(k))
    out.update(precision=pr["precision"], recall=pr["recall"], f1=pr["f1"])
    if kid:
        out.update(kid_mean=kid[0], kid_std=kid[1])
    if ndb is not None:
        st = ndb_statistics(bins[0], bins[1], ndb[1])
        out.update(ndb=st["ndb"], ndb_over_k=st["ndb_over_k"], js_divergence=st["js_divergence"])
    if spec is not None:
        out.update(_spectrum_result(spec, sp))
    return out


def _spectrum_result(spec, sums) -> Dict[str, float]:
    """The four spectral keys from the two running sums read in the pass's host sync (real first, then fake)."""
    nb = spec[0].plan.n_bins
    d = _spectral_distance(spec[0].plan, np.asarray(sums[:nb]) / spec[0].n, np.asarray(sums[nb:]) / spec[1].n, 1, 0.5)
    return {key: d[key] for key in ("lsd_db", "hf_excess_db", "hf_share_real", "hf_share_fake")}


@torch.no_grad()
def sample_images(decoder, z: Optional[torch.Tensor] = None, n: int = 64,
                  prior: Optional[Union[LatentPrior, GaussianMixturePrior]] = None,
                  grid_cols: int = 0) -> torch.Tensor:
    """Generated images as uint8 on the device ((fake + 1) / 2 * 255, clamped and truncated: main_vae.py:492,498-499), the
    decoder in eval mode:
        z=None, prior=None: n images from z ~ N(0, I)                        (sample_vae_decoder, main_vae.py:364-366)
        z f32 [n, nz, 1, 1]: the images of that z -- the per-epoch ``decoder(fixed_noise)`` picture, vaegan_code.py:40, 209-216
        prior:              n images from the histogram prior                (sample_vae, main_vae.py:619-626)
                            or from a GaussianMixturePrior (any object with ``sample_z(n, decoder)``)
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
    return ops.to_u8(decoder.decode_eval(zh, n), grid_cols)
