"""numpy f64 restatement of the Gaussian-mixture prior, written from include/vaegan_hip.h ("Gaussian-mixture prior") and
from the docstring of latent.GaussianMixturePrior.fit: the E-step, the shifted one-pass M-step sums, the host part of the
M-step, the EM loop of scikit-learn's GaussianMixture.fit, and the sampler.  x is always f32; every operation is f64 on the
exactly converted values."""
import numpy as np
from scipy import linalg

TINY = 10 * np.finfo(np.float64).eps


def log_resp(x, mean, prec_chol, log_coef):
    """-> (log_prob [N,K], log_norm [N], resp [N,K])."""
    assert x.dtype == np.float32
    x64 = x.astype(np.float64)
    N, K = x.shape[0], mean.shape[0]
    lp = np.empty((N, K))
    for k in range(K):
        y = (x64 - mean[k]) @ np.triu(prec_chol[k])
        lp[:, k] = log_coef[k] - 0.5 * np.sum(y * y, axis=1)
    m = lp.max(axis=1)
    s = np.zeros(N)
    for k in range(K):                                                   # k ascending
        s = s + np.exp(lp[:, k] - m)
    ln = m + np.log(s)
    return lp, ln, np.exp(lp - ln[:, None])


def moments(x, shift, resp, log_norm=None):
    """-> (nk [K], s1 [K,D], s2 [K,D,D], loglik_sum or None) with d = x - shift_k."""
    assert x.dtype == np.float32
    x64 = x.astype(np.float64)
    K, D = shift.shape
    nk = resp.sum(axis=0)
    s1 = np.empty((K, D))
    s2 = np.empty((K, D, D))
    for k in range(K):
        d = x64 - shift[k]
        rd = resp[:, k, None] * d
        s1[k] = rd.sum(axis=0)
        s2[k] = rd.T @ d
    return nk, s1, s2, (None if log_norm is None else log_norm.sum())


def moments_abs(x, shift, resp):
    """sum of the absolute values of the terms of s1 and s2: the scale of their rounding-error bound."""
    x64 = x.astype(np.float64)
    K, D = shift.shape
    a1 = np.empty((K, D))
    a2 = np.empty((K, D, D))
    for k in range(K):
        d = np.abs(x64 - shift[k])
        rd = np.abs(resp[:, k, None]) * d
        a1[k] = rd.sum(axis=0)
        a2[k] = rd.T @ d
    return a1, a2


def global_variance(x, row):
    """Per-column variance of x from ONE moments call with K = 1, resp = 1, shift = x[row]."""
    N = x.shape[0]
    nk, s1, s2, _ = moments(x, x[row:row + 1].astype(np.float64), np.ones((N, 1)))
    delta = s1[0] / nk[0]
    return np.diagonal(s2[0]) / nk[0] - delta * delta


def m_step(n, shift, nk, s1, s2, reg_covar):
    """The host part of the M-step -> dict(weights, means, covariances, cov_chol, prec_chol, log_coef, cdf).
    Raises numpy.linalg.LinAlgError where a covariance is not positive definite."""
    K, D = shift.shape
    nk = nk + TINY
    weights = nk / n
    weights = weights / weights.sum()
    delta = s1 / nk[:, None]
    means = shift + delta
    cov = s2 / nk[:, None, None] - delta[:, :, None] * delta[:, None, :]
    cov = 0.5 * (cov + cov.transpose(0, 2, 1))
    cov[:, np.arange(D), np.arange(D)] += reg_covar
    return finish(weights, means, cov)


def finish(weights, means, cov):
    K, D = means.shape
    cov_chol = np.empty_like(cov)
    prec_chol = np.empty_like(cov)
    for k in range(K):
        if not np.all(np.isfinite(cov[k])):
            raise np.linalg.LinAlgError("covariance is not finite")
        cov_chol[k] = linalg.cholesky(cov[k], lower=True)
        prec_chol[k] = linalg.solve_triangular(cov_chol[k], np.eye(D), lower=True).T
    log_det = np.log(np.diagonal(prec_chol, axis1=1, axis2=2)).sum(axis=1)
    log_coef = np.log(weights) + log_det - 0.5 * D * np.log(2.0 * np.pi)
    return dict(weights=weights, means=means, covariances=cov, cov_chol=cov_chol, prec_chol=prec_chol, log_coef=log_coef,
                cdf=np.cumsum(weights))


def init_params(x, init_idx, reg_covar):
    """Means = the rows init_idx, weights 1/K, every precision diag(1 / (var + reg_covar))."""
    init_idx = np.asarray(init_idx)
    K, D = len(init_idx), x.shape[1]
    var = global_variance(x, int(init_idx[0]))
    prec = 1.0 / (var + reg_covar)
    means = x[init_idx].astype(np.float64)
    weights = np.full(K, 1.0 / K)
    prec_chol = np.tile(np.diag(np.sqrt(prec)), (K, 1, 1))
    log_coef = np.log(weights) + np.log(np.sqrt(prec)).sum() - 0.5 * D * np.log(2.0 * np.pi)
    return dict(weights=weights, means=means, prec_chol=prec_chol, log_coef=log_coef, precisions=np.tile(np.diag(prec), (K, 1, 1)))


def fit(x, init_idx, reg_covar=1e-6, tol=1e-3, max_iter=100, e_step=log_resp, m_sums=moments):
    """scikit-learn's GaussianMixture.fit loop with the shifted one-pass M-step.  e_step / m_sums: the two device phases
    (replaceable, so the same loop can run them elsewhere).  -> dict of parameters + converged, n_iter, lower_bound."""
    N = x.shape[0]
    p = init_params(x, init_idx, reg_covar)
    lower, converged, n_iter = -np.inf, False, 0
    for n_iter in range(1, max_iter + 1):
        prev = lower
        _, ln, resp = e_step(x, p["means"], p["prec_chol"], p["log_coef"])
        nk, s1, s2, ll = m_sums(x, p["means"], resp, ln)
        lower = float(ll) / N
        if not np.isfinite(lower):
            raise np.linalg.LinAlgError("lower bound is not finite")
        p = m_step(N, p["means"], nk, s1, s2, reg_covar)
        if abs(lower - prev) < tol:
            converged = True
            break
    p.update(converged=converged, n_iter=n_iter, lower_bound=lower)
    return p


def sample(cdf, mean, cov_chol, u, eps):
    """u f64 [n], eps f32 [n,D] -> (comp int32 [n], z64 [n,D], z32 f32 [n,D]); the sums in the header's order."""
    n, D = eps.shape
    K = len(cdf)
    comp = np.minimum(np.searchsorted(cdf, u, side="right"), K - 1).astype(np.int32)
    z64 = np.empty((n, D))
    e64 = eps.astype(np.float64)
    for j in range(n):
        Lk = np.tril(cov_chol[comp[j]])
        z64[j] = mean[comp[j]] + Lk @ e64[j]
    return comp, z64, z64.astype(np.float32)


# ---- shared inputs ---------------------------------------------------------------------------------------------------
# (N, D, K, offset) of the fit comparisons; SKLEARN_MEASURED is the largest relative deviation of `fit` from scikit-learn's
# GaussianMixture over these cases (tests/test_gmm_cpu.py measures and prints it); FIT_BOUND = 64 x that is asserted both
# there and for the device fit against `fit` (f64 EM in another summation order, the same kind of difference).
FIT_CASES = ((2000, 8, 3, 0.0), (4096, 20, 4, 0.0), (600, 5, 2, 0.0), (3000, 100, 4, 0.0), (2000, 8, 3, 100.0))
SKLEARN_MEASURED = 1.15e-12
FIT_BOUND = 64 * SKLEARN_MEASURED


def make_mixture(N, D, K, offset=0.0):
    """f32 [N, D] rows of K overlapping full-covariance Gaussians (centres ~ 1.2 N(0, I)), shifted by `offset`."""
    r = np.random.default_rng(N + D)
    cen = r.normal(size=(K, D)) * 1.2
    A = r.normal(size=(K, D, D)) / np.sqrt(D) + np.eye(D) * 0.5
    lab = r.integers(0, K, N)
    x = cen[lab] + np.einsum("nij,nj->ni", A[lab], r.normal(size=(N, D)))
    return (x + offset).astype(np.float32)


def default_init(N, K, seed=0):
    return np.random.default_rng(seed).choice(N, K, replace=False)


def rel_dev(a, b):
    """Largest deviation relative to the largest magnitude of the reference b."""
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def exact_estep_inputs(N, D, K, seed=0):
    """Integer x and means with |.| <= 3, upper-triangular U with entries in {0, +-0.5, +-1, 2}, dyadic log_coef: every
    intermediate of log_prob is exactly representable in f64, whatever the order of the additions."""
    r = np.random.default_rng(1000 * seed + 7 * N + 3 * D + K)
    x = r.integers(-3, 4, (N, D)).astype(np.float32)
    mean = r.integers(-3, 4, (K, D)).astype(np.float64)
    U = np.triu(r.choice(np.array([0.0, 0.5, -0.5, 1.0, -1.0, 2.0]), (K, D, D)))
    log_coef = r.integers(-32, 33, K) / 8.0
    return x, mean, U, log_coef


def exact_moment_inputs(N, D, K, seed=0):
    """Integer x and shift with |.| <= 3, resp rows of multiples of 1/8 summing to 1, log_norm multiples of 1/4."""
    r = np.random.default_rng(2000 * seed + 7 * N + 3 * D + K)
    x = r.integers(-3, 4, (N, D)).astype(np.float32)
    shift = r.integers(-3, 4, (K, D)).astype(np.float64)
    e = np.zeros((N, K), np.int64)
    for _ in range(8):                                                   # eight eighths per row, thrown at the components
        np.add.at(e, (np.arange(N), r.integers(0, K, N)), 1)
    log_norm = r.integers(-32, 1, N) / 4.0
    return x, shift, e / 8.0, log_norm


def exact_sample_inputs(n, D, K, seed=0):
    """Dyadic means and lower factors, dyadic eps; u hits 0, every cdf entry, 1 - 2^-24 and the clamp (the cdf's last
    entry is 1 - 2^-53 and one u equals it)."""
    r = np.random.default_rng(3000 * seed + 7 * n + 3 * D + K)
    mean = r.integers(-16, 17, (K, D)) / 4.0
    chol = np.tril(r.choice(np.array([0.0, 0.25, 0.5, -0.5, 1.0, -1.0, 2.0]), (K, D, D)))
    eps = (r.integers(-32, 33, (n, D)) / 8.0).astype(np.float32)
    cdf = np.arange(1, K + 1) / K
    cdf[-1] = 1.0 - 2.0 ** -53
    special = np.concatenate([[0.0, 1.0 - 2.0 ** -24, 1.0 - 2.0 ** -53], cdf])
    u = r.random(n)
    m = min(n, len(special))
    u[:m] = special[:m]
    return cdf, mean, chol, u, eps
