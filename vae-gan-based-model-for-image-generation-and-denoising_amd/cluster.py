"""K-means on the device: Lloyd's iteration with k-means++ seeding over feature or latent rows that already sit in HBM
(not in the reference).  It is the primitive behind two things of the generation side: the k-means start of
``latent.GaussianMixturePrior.fit(init="kmeans")`` (scikit-learn's ``init_params="kmeans"``, what Ghosh et al. 2020 use for
ex-post density estimation) and the bins of ``metrics.ndb`` (Richardson & Weiss 2018).  The kernels are stated in
include/vaegan_hip.h, "K-means": vg_kmeans_assign (the N x K x D scores on the f64 MFMA, lowest k on a tie),
vg_kmeans_update (counts, sums, centres over a fixed row split) and vg_kmeans_seed (plain k-means++, no host sync).

Out of scope: scikit-learn's greedy k-means++ trials and ``n_init > 1`` (loop over seeds and keep the lowest
``inertia_``), empty-cluster relocation (an empty cluster keeps its centre), sample weights, Elkan's algorithm.
"""
from typing import Dict, Optional

import numpy as np
import torch

from . import ops

_KM_KEYS = ("cluster_centers_", "counts_")


class KMeans:
    """A fitted k-means clustering.  Device tensors: ``cluster_centers_`` f64 [K, D], ``counts_`` int64 [K] (rows per
    cluster under the final labels), ``labels_`` int32 [N] (None on a loaded object).  Python values: ``inertia_`` (sum of
    squared distances to the final centres), ``n_iter_``, ``converged``, ``n_fitted``, ``n_clusters``, ``dim``."""

    def __init__(self, cluster_centers_, counts_, labels_=None, inertia_: float = float("nan"), n_iter_: int = 0,
                 converged: bool = True, n_fitted: int = 0):
        for t in (cluster_centers_, counts_, labels_):
            if t is not None and not t.is_cuda:
                raise RuntimeError("KMeans lives on the MI355X ('cuda'); there is no CPU path")
        K, D = (cluster_centers_.shape[0], cluster_centers_.shape[1]) if cluster_centers_.dim() == 2 else (0, 0)
        if (K < 1 or D < 1 or cluster_centers_.dtype != torch.float64 or counts_.dtype != torch.int64
                or tuple(counts_.shape) != (K,)):
            raise RuntimeError("KMeans: f64 cluster_centers_ [K, D] and int64 counts_ [K]")
        self.cluster_centers_, self.counts_, self.labels_ = cluster_centers_.contiguous(), counts_.contiguous(), labels_
        self.n_clusters, self.dim = K, D
        self.inertia_, self.n_iter_ = float(inertia_), int(n_iter_)
        self.converged, self.n_fitted = bool(converged), int(n_fitted)

    @classmethod
    def fit(cls, x: torch.Tensor, n_clusters: int, init="k-means++", max_iter: int = 300, tol: float = 1e-4, seed: int = 0,
            u: Optional[torch.Tensor] = None) -> "KMeans":
        """Lloyd's iteration on x f32 [N, D] on the device, possibly a strided view (``mulv[:, :L]``: no copy is made).

        init: ``"k-means++"`` -- ``ops.kmeans_seed`` with the draws ``u`` (f64 [K] on the device) or, by default, those of
        the device generator at state {seed, 0}; K distinct row numbers (a sequence or array of integers); or an f64
        [K, D] device tensor of centres.
        Loop: scikit-learn's ``_kmeans_single_lloyd`` -- assign every row to its nearest centre, move every centre to the
        mean of its rows; stop when no label changed (strict) or when the summed squared centre shift is <= ``tol`` times
        the mean per-column variance of x (one ``ops.gmm_moments`` call with K = 1); after a non-strict stop the rows are
        assigned once more, and ``inertia_`` is taken against the final centres.  Per iteration: ``ops.kmeans_assign``,
        ``ops.kmeans_update`` and ONE host sync reading three numbers.  Deviation: an empty cluster keeps its centre.
        RuntimeError: host tensors, a wrong dtype or rank, K or D outside the limits, N < K, duplicate seed rows (fewer
        than K distinct rows under k-means++), a non-finite inertia (a NaN or infinite row)."""
        if not x.is_cuda:
            raise RuntimeError("KMeans.fit needs the rows on the MI355X ('cuda'); there is no CPU path")
        if x.dim() != 2 or x.dtype != torch.float32:
            raise RuntimeError("KMeans.fit: x must be f32 [N, D]")
        N, D = x.shape
        K = int(n_clusters)
        if not (1 <= K <= ops.KMEANS_MAX_K and 1 <= D <= ops.KMEANS_MAX_D):
            raise RuntimeError(f"KMeans.fit: needs 1 <= n_clusters <= {ops.KMEANS_MAX_K} and 1 <= D <= {ops.KMEANS_MAX_D}")
        if N < K:
            raise RuntimeError(f"KMeans.fit: {N} rows cannot seed {K} clusters")
        if int(max_iter) < 1:
            raise RuntimeError("KMeans.fit: max_iter must be >= 1")
        if isinstance(init, str):
            if init != "k-means++":
                raise RuntimeError(f"KMeans.fit: init must be 'k-means++', K row numbers or f64 [K, D] centres, got {init!r}")
            dev = x.device
            if u is not None:
                if not u.is_cuda:
                    raise RuntimeError("KMeans.fit needs the draws u on the MI355X ('cuda'); there is no CPU path")
                _, centers, _ = ops.kmeans_seed(x, K, u=u)
            else:
                state = torch.tensor([int(seed), 0], dtype=torch.int64, device=dev)
                _, centers, _ = ops.kmeans_seed(x, K, state=state)
            if np.unique(centers.cpu().numpy(), axis=0).shape[0] != K:
                raise RuntimeError(f"KMeans.fit: k-means++ found fewer than {K} distinct rows (duplicate seed rows); "
                                   f"ask for fewer clusters")
        elif isinstance(init, torch.Tensor) and init.is_floating_point():
            if not init.is_cuda:
                raise RuntimeError("KMeans.fit needs the initial centres on the MI355X ('cuda'); there is no CPU path")
            if init.dtype != torch.float64 or tuple(init.shape) != (K, D):
                raise RuntimeError(f"KMeans.fit: initial centres must be f64 [{K}, {D}]")
            centers, dev = init.contiguous().clone(), x.device
        else:
            idx = np.asarray(init.cpu() if isinstance(init, torch.Tensor) else init)
            if (idx.ndim != 1 or idx.size != K or not np.issubdtype(idx.dtype, np.integer) or idx.min() < 0
                    or idx.max() >= N or np.unique(idx).size != K):
                raise RuntimeError(f"KMeans.fit: init must be {K} distinct row numbers in [0, {N}) (duplicate seed rows are "
                                   f"refused)")
            dev = x.device
            centers = x[torch.as_tensor(idx, dtype=torch.int64, device=dev)].double().contiguous()
        # tol is relative to the mean per-column variance, as in scikit-learn's _tolerance
        nk, s1, s2, _ = ops.gmm_moments(x, x[:1].double().contiguous(), torch.ones(N, 1, dtype=torch.float64, device=dev))
        flat = torch.cat([nk, s1.reshape(-1), torch.diagonal(s2[0])]).cpu().numpy()
        delta = flat[1:1 + D] / flat[0]
        scaled_tol = float(np.mean(flat[1 + D:] / flat[0] - delta * delta)) * float(tol)
        prev = torch.full((N,), -1, dtype=torch.int32, device=dev)
        strict = converged = False
        n_iter, inertia, count, label = 0, float("nan"), None, None
        for n_iter in range(1, int(max_iter) + 1):
            label, dist2, _, changed = ops.kmeans_assign(x, centers, want_dist2=True, prev_label=prev)
            count, _, centers, stats = ops.kmeans_update(x, label, K, old=centers, dist2=dist2)
            n_changed, shift2, inertia = torch.cat([changed.double(), stats]).tolist()       # the one host sync
            if not np.isfinite(inertia):
                raise RuntimeError(f"KMeans.fit: the inertia is not finite in iteration {n_iter} (a NaN or infinite row)")
            if n_changed == 0:
                strict = converged = True
                break
            if shift2 <= scaled_tol:
                converged = True
                break
            prev = label
        if not strict:
            label, dist2, _, _ = ops.kmeans_assign(x, centers, want_dist2=True)
            count, _, _, stats = ops.kmeans_update(x, label, K, dist2=dist2)
            inertia = float(stats[1].item())
            if not np.isfinite(inertia):
                raise RuntimeError("KMeans.fit: the final inertia is not finite (a NaN or infinite row)")
        return cls(centers, count, label, inertia_=inertia, n_iter_=n_iter, converged=converged, n_fitted=N)

    def predict(self, x: torch.Tensor) -> torch.Tensor:
        """The nearest centre of every row of x f32 [N, D] (device) -> int32 [N]; one launch, no host sync."""
        if not x.is_cuda:
            raise RuntimeError("KMeans.predict needs the rows on the MI355X ('cuda'); there is no CPU path")
        if x.dim() != 2 or x.shape[1] != self.dim:
            raise RuntimeError(f"KMeans.predict: x must be [N, {self.dim}]")
        return ops.kmeans_assign(x, self.cluster_centers_)[0]

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """Plain tensors (without the N labels): cluster the real features once, save, reuse for every checkpoint."""
        sd = {k: getattr(self, k) for k in _KM_KEYS}
        sd.update(inertia_=torch.tensor(self.inertia_, dtype=torch.float64), n_iter_=torch.tensor(self.n_iter_),
                  converged=torch.tensor(self.converged), n_fitted=torch.tensor(self.n_fitted))
        return sd

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> "KMeans":
        """Replace this clustering by that of ``sd`` (a ``state_dict()``, e.g. from torch.load), moved to its device."""
        dev = self.cluster_centers_.device
        self.__init__(*(sd[k].to(dev) for k in _KM_KEYS), None, inertia_=float(sd["inertia_"]), n_iter_=int(sd["n_iter_"]),
                      converged=bool(sd["converged"]), n_fitted=int(sd["n_fitted"]))
        return self

    @classmethod
    def from_state_dict(cls, sd: Dict[str, torch.Tensor], device="cuda") -> "KMeans":
        return cls(*(sd[k].to(device) for k in _KM_KEYS), None, inertia_=float(sd["inertia_"]), n_iter_=int(sd["n_iter_"]),
                   converged=bool(sd["converged"]), n_fitted=int(sd["n_fitted"]))
