"""f64 numpy restatement of the feature-space metrics (include/vaegan_hip.h "Feature-space metrics", metrics.py): the
yardstick of tests/test_metrics_cpu.py and tests/test_gpu_metrics.py.  Brute force on purpose: distances by direct
differences, np.partition, np.linalg.eigvals; nothing here calls the package."""
import numpy as np


def stats(x):
    """x [n, D] (any float dtype) -> (sum f64 [D], outer f64 [D, D], n): torchmetrics' running sums of features.double()."""
    x = np.asarray(x, np.float64)
    return x.sum(0), x.T @ x, x.shape[0]


def mean_cov(s, o, n):
    """torchmetrics FrechetInceptionDistance.compute: mean = sum / n, cov = (outer - n mean^T mean) / (n - 1)."""
    m = s / n
    return m, (o - n * np.outer(m, m)) / (n - 1)


def fid_from_moments(m1, c1, m2, c2):
    """torchmetrics _compute_fid: |m1 - m2|^2 + tr c1 + tr c2 - 2 sum Re sqrt(eigvals(c1 c2))."""
    d = m1 - m2
    ev = np.linalg.eigvals(c1 @ c2).astype(np.complex128)
    return float(d @ d + np.trace(c1) + np.trace(c2) - 2.0 * np.sqrt(ev).real.sum())


def fid_sqrtm(m1, c1, m2, c2):
    """The classic form (Heusel et al. 2017): tr sqrtm(c1 c2) by scipy."""
    from scipy.linalg import sqrtm
    d = m1 - m2
    return float(d @ d + np.trace(c1) + np.trace(c2) - 2.0 * np.trace(sqrtm(c1 @ c2)).real)


def fid(real, fake):
    """FID of two feature matrices [n, D]."""
    return fid_from_moments(*mean_cov(*stats(real)), *mean_cov(*stats(fake)))


def dist2(a, b, chunk=64):
    """Squared Euclidean distances [len(a), len(b)] in f64 by direct differences."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.empty((a.shape[0], b.shape[0]), np.float64)
    for i in range(0, a.shape[0], chunk):
        d = a[i:i + chunk, None, :] - b[None, :, :]
        out[i:i + chunk] = np.einsum("ijk,ijk->ij", d, d)
    return out


def knn_radius2(x, k):
    """k-th smallest squared distance from row i to the OTHER rows (row i excluded by index: a duplicate row counts)."""
    d = dist2(x, x)
    np.fill_diagonal(d, np.inf)
    return np.partition(d, k - 1, axis=1)[:, k - 1]


def cover(q, ref, r2_ref):
    """bool [len(q)]: q_i lies inside the ball of squared radius r2_ref[j] around some ref_j."""
    return (dist2(q, ref) <= np.asarray(r2_ref, np.float64)[None, :]).any(1)


def precision_recall(real, fake, k=3):
    p = float(cover(fake, real, knn_radius2(real, k)).mean())
    r = float(cover(real, fake, knn_radius2(fake, k)).mean())
    return {"precision": p, "recall": r, "f1": 0.0 if p + r == 0 else 2 * p * r / (p + r),
            "n_real": len(real), "n_fake": len(fake), "k": k}


# ---- error bounds of the f32 GEMM-form distance (the header's 2 (D + 4) 2^-24 (|a|^2 + |b|^2)) -------------------------
def dist_tol(a, b):
    """tol[i, j] = 2 (D + 4) 2^-24 (|a_i|^2 + |b_j|^2)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    D = a.shape[1]
    return 2.0 * (D + 4) * 2.0 ** -24 * ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :])


def decided_cover(q, ref, r2_ref):
    """-> (inside bool [Nq], decided bool [Nq]).  A sample is decided when it is inside by more than 2 tol for some j, or
    outside by more than 2 tol for every j (one tol for the distance, one for the radius the device computed itself)."""
    d = dist2(q, ref)
    t = 2.0 * dist_tol(q, ref)
    r = np.asarray(r2_ref, np.float64)[None, :]
    surely_in = (d < r - t).any(1)
    surely_out = (d > r + t).all(1)
    return (d <= r).any(1), surely_in | surely_out
