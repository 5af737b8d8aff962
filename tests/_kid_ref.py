"""f64 numpy restatement of the Kernel Inception Distance (include/vaegan_hip.h, vg_kid_scores; metrics.kernel_distance):
the yardstick of tests/test_kid_cpu.py and tests/test_gpu_kid.py.  Brute force on purpose: the full m x m Gram matrices
that the kernel never writes.  Nothing here calls the package.  Also the input generators and the error bounds of the GPU
tests, so that the CPU tests can exercise them too."""
import numpy as np

U = 2.0 ** -53                      # unit roundoff of f64


def poly_kernel(a, c, degree, gamma, coef):
    """k[i, j] = (gamma a_i . c_j + coef)^degree, the power as degree - 1 left-to-right multiplications (no pow)."""
    base = gamma * (np.asarray(a, np.float64) @ np.asarray(c, np.float64).T) + coef
    k = base.copy()
    for _ in range(int(degree) - 1):
        k = k * base
    return k


def _off_diagonal_sum(k):
    k = k.copy()
    np.fill_diagonal(k, 0.0)        # left out by POSITION in the subset
    return float(k.sum())


def poly_mmd_sums(x, y, degree, gamma, coef):
    """x, y [m, D] -> (sum_{i != j} k(x_i, x_j), sum_{i != j} k(y_i, y_j), sum_{i, j} k(x_i, y_j))."""
    return (_off_diagonal_sum(poly_kernel(x, x, degree, gamma, coef)),
            _off_diagonal_sum(poly_kernel(y, y, degree, gamma, coef)), float(poly_kernel(x, y, degree, gamma, coef).sum()))


def score_from_sums(s0, s1, s2, m):
    m = float(m)
    return (s0 + s1) / (m * (m - 1.0)) - 2.0 * s2 / (m * m)


def kid(real, fake, idx_real, idx_fake, degree=3, gamma=None, coef=1.0):
    """-> (scores f64 [S], mean, population std, sums f64 [S, 3]); subset s = real[idx_real[s]], fake[idx_fake[s]]."""
    real, fake = np.asarray(real, np.float64), np.asarray(fake, np.float64)
    gamma = 1.0 / real.shape[1] if gamma is None else float(gamma)
    S, m = np.asarray(idx_real).shape
    sums = np.empty((S, 3), np.float64)
    for s in range(S):
        sums[s] = poly_mmd_sums(real[np.asarray(idx_real)[s]], fake[np.asarray(idx_fake)[s]], degree, gamma, coef)
    scores = np.array([score_from_sums(*sums[s], m) for s in range(S)])
    mean, std = mean_std(scores)
    return scores, mean, std, sums


def mean_std(scores):
    """Mean (added in ascending order) and population standard deviation sqrt(sum (score - mean)^2 / S)."""
    tot = 0.0
    for v in scores:
        tot += float(v)
    mean = tot / len(scores)
    var = 0.0
    for v in scores:
        var += (float(v) - mean) ** 2
    return mean, float(np.sqrt(var / len(scores)))


# ---- inputs -----------------------------------------------------------------------------------------------------------
def gauss_feats(n, D, seed, mix=True):
    """f32 [n, D]: correlated Gaussian columns of mixed scale with offsets (the generator of test_gpu_metrics.py)."""
    g = np.random.default_rng(seed)
    x = g.standard_normal((n, D))
    if mix and D > 1:
        x = x @ (np.eye(D) + 0.3 * g.standard_normal((D, D)) / np.sqrt(D))
    return (x * g.uniform(0.5, 2.0, D) + g.uniform(-1, 1, D)).astype(np.float32)


def int_feats(n, D, seed):
    """f32 [n, D] of integers in [-3, 3]: with gamma = coef = 1 every intermediate of the metric is an integer."""
    return np.random.default_rng(seed).integers(-3, 4, (n, D)).astype(np.float32)


def tables(N, S, m, seed):
    """int32 [S, m]: each row a duplicate-free draw from range(N), no particular order."""
    g = np.random.default_rng(seed)
    return np.stack([g.permutation(N)[:m] for _ in range(S)]).astype(np.int32)


# ---- bounds -----------------------------------------------------------------------------------------------------------
def sum_bounds(x, y, degree, gamma, coef):
    """Bound on |computed - exact| for the three sums of one subset, doubled: see test_gpu_kid.py's docstring.
        Bbar_ij = |gamma| sum_c |a_c b_c| + |coef|;   n_f = number of terms;
        |d sum| <= 2 (degree (D + 3) + n_f) u sum Bbar_ij^degree"""
    x, y = np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(y, np.float64))
    m, D = x.shape
    out = []
    for a, c, off in ((x, x, True), (y, y, True), (x, y, False)):
        bb = (abs(gamma) * (a @ c.T) + abs(coef)) ** int(degree)
        if off:
            np.fill_diagonal(bb, 0.0)
        n_f = m * (m - 1) if off else m * m
        out.append(2.0 * (degree * (D + 3) + n_f) * U * float(bb.sum()))
    return np.array(out)


def score_bound(sums, dsums, m):
    """The sums' bounds through scores = (s0 + s1) / (m (m - 1)) - 2 s2 / m^2, plus 4 u per term for the formula's own
    roundings (an addition, two divisions, a subtraction; on both sides of the comparison)."""
    m = float(m)
    t1, t2 = abs(sums[0] + sums[1]) / (m * (m - 1.0)), 2.0 * abs(sums[2]) / (m * m)
    return (dsums[0] + dsums[1]) / (m * (m - 1.0)) + 2.0 * dsums[2] / (m * m) + 4.0 * U * (t1 + t2)


def kid_bounds(real, fake, idx_real, idx_fake, degree, gamma, coef):
    """-> (dsums [S, 3], dscores [S]) for the restatement's own sums of the same subsets."""
    real, fake = np.asarray(real, np.float64), np.asarray(fake, np.float64)
    S, m = np.asarray(idx_real).shape
    _, _, _, sums = kid(real, fake, idx_real, idx_fake, degree, gamma, coef)
    ds = np.stack([sum_bounds(real[idx_real[s]], fake[idx_fake[s]], degree, gamma, coef) for s in range(S)])
    return ds, np.array([score_bound(sums[s], ds[s], m) for s in range(S)])
