"""numpy f64 restatement of the k-means entry points, written from include/vaegan_hip.h ("K-means") and from the
docstrings of cluster.KMeans.fit, latent.GaussianMixturePrior.fit(init=) and metrics.ndb: the scores and the tie rule,
direct-form dist2, the update, the two-level cumulative sum of the k-means++ seeding, the Lloyd loop of scikit-learn's
_kmeans_single_lloyd, the k-means start of the mixture prior (on _gmm_ref's functions) and the NDB arithmetic.  x is always
f32; every operation is f64 on the exactly converted values."""
import math

import numpy as np

import _gmm_ref as G

SEED_BLOCK = 256
EPS = 2.0 ** -53


# ---- assignment ---------------------------------------------------------------------------------------------------
def scores(x, c):
    """s[n, k] = 0.5 |c_k|^2 - x_n . c_k  -> [N, K]."""
    assert x.dtype == np.float32 and c.dtype == np.float64
    return 0.5 * np.sum(c * c, axis=1)[None, :] - x.astype(np.float64) @ c.T


def score_scale(x, c):
    """0.5 |c_k|^2 + sum_i |x_i| |c_ki|: the sum of the magnitudes of a score's terms, the scale of its rounding error."""
    return 0.5 * np.sum(c * c, axis=1)[None, :] + np.abs(x.astype(np.float64)) @ np.abs(c).T


def assign(x, c):
    """-> (label int32 [N] = the lowest k with minimal score, 0 for a row with a NaN; dist2 [N] direct form; gap [N] =
    second-best minus best score, inf where K = 1)."""
    s = scores(x, c)
    bad = np.isnan(s).any(axis=1)
    s0 = np.where(bad[:, None], 0.0, s)
    label = np.argmin(s0, axis=1).astype(np.int32)                      # the first minimum: the lowest k
    d = x.astype(np.float64) - c[label]
    dist2 = np.sum(d * d, axis=1)
    if c.shape[0] > 1:
        part = np.partition(s0, 1, axis=1)
        gap = part[:, 1] - part[:, 0]
    else:
        gap = np.full(x.shape[0], np.inf)
    return label, dist2, gap


def one_hot(label, K):
    r = np.zeros((len(label), K))
    ok = (label >= 0) & (label < K)
    r[np.nonzero(ok)[0], label[ok]] = 1.0
    return r


# ---- update -------------------------------------------------------------------------------------------------------
def update(x, label, K, old=None, dist2=None):
    """-> (count int64 [K], sum [K, D], center [K, D] or None, stats [2]); labels outside [0, K) are skipped; an empty
    cluster keeps its old centre."""
    x64 = x.astype(np.float64)
    D = x.shape[1]
    ok = (label >= 0) & (label < K)
    count = np.bincount(label[ok], minlength=K).astype(np.int64)
    s = np.zeros((K, D))
    np.add.at(s, label[ok], x64[ok])
    center, shift2 = None, 0.0
    if old is not None:
        center = old.copy()
        nz = count > 0
        center[nz] = s[nz] / count[nz, None].astype(np.float64)
        for k in range(K):
            row = 0.0
            for v in (center[k] - old[k]) ** 2:
                row += v
            shift2 += row
    return count, s, center, np.array([shift2, 0.0 if dist2 is None else float(np.sum(dist2))])


# ---- seeding ------------------------------------------------------------------------------------------------------
def _sq_dist_rows(x64, row):
    d = np.zeros(x64.shape[0])
    for i in range(x64.shape[1]):                                        # columns ascending
        e = x64[:, i] - row[i]
        d = d + e * e
    return d


def seed(x, K, u, block=SEED_BLOCK):
    """Plain k-means++ with the header's two-level cumulative sum.  -> (idx int32 [K], center [K, D], mind2 [N], gap): gap is
    the smallest distance of a target u_j * total to the cumulative boundaries on either side of the picked row, relative
    to total (inf where K = 1) -- how far the inputs are from a pick that rounding could move."""
    x64 = x.astype(np.float64)
    N = x.shape[0]
    idx = np.empty(K, np.int64)
    idx[0] = min(int(u[0] * N), N - 1)
    mind2 = _sq_dist_rows(x64, x64[idx[0]])
    gap = np.inf
    nb = (N + block - 1) // block
    for j in range(1, K):
        pad = np.zeros(nb * block)
        pad[:N] = mind2
        btot = np.cumsum(pad.reshape(nb, block), axis=1)[:, -1]          # rows ascending inside a block
        cumb = np.cumsum(btot)                                           # block totals ascending
        total = cumb[-1]
        target = u[j] * total
        hit = np.nonzero(cumb > target)[0]
        if hit.size == 0:
            idx[j] = N - 1
        else:
            b = int(hit[0])
            prefix = cumb[b - 1] if b > 0 else 0.0
            cum = prefix + np.cumsum(pad[b * block:(b + 1) * block])    # the block's own running sum, then ONE addition
            q = int(np.nonzero(cum > target)[0][0])
            idx[j] = min(b * block + q, N - 1)
            below = cum[q - 1] if q > 0 else prefix
            if total > 0:
                gap = min(gap, (cum[q] - target) / total, (target - below) / total if target > below else np.inf)
        mind2 = np.minimum(mind2, _sq_dist_rows(x64, x64[idx[j]]))
    return idx.astype(np.int32), x64[idx], mind2, gap


# ---- Lloyd --------------------------------------------------------------------------------------------------------
def lloyd(x, centers, max_iter=300, tol=1e-4):
    """scikit-learn's _kmeans_single_lloyd from the given centres (an empty cluster keeps its centre) -> dict(centers,
    labels, inertia, n_iter, counts, converged, min_gap, emptied)."""
    N = x.shape[0]
    K = centers.shape[0]
    scaled_tol = float(np.mean(G.global_variance(x, 0))) * tol
    c = centers.astype(np.float64).copy()
    prev = np.full(N, -1, np.int32)
    strict = converged = emptied = False
    min_gap, n_iter = np.inf, 0
    for n_iter in range(1, max_iter + 1):
        label, dist2, gap = assign(x, c)
        min_gap = min(min_gap, float(gap.min()))
        count, _, c, stats = update(x, label, K, old=c, dist2=dist2)
        emptied = emptied or bool(np.any(count == 0))
        if np.array_equal(label, prev):
            strict = converged = True
            break
        if stats[0] <= scaled_tol:
            converged = True
            break
        prev = label
    if not strict:
        label, dist2, gap = assign(x, c)
        min_gap = min(min_gap, float(gap.min()))
        count = np.bincount(label, minlength=K).astype(np.int64)
    return dict(centers=c, labels=label, inertia=float(np.sum(dist2)), n_iter=n_iter, counts=count, converged=converged,
                min_gap=min_gap, emptied=emptied)


# ---- the k-means start of the mixture prior ---------------------------------------------------------------------------
def gmm_start(x, centers, reg_covar=1e-6):
    """scikit-learn's init_params="kmeans": the M-step on the one-hot responsibilities of the rows' nearest centres."""
    label, _, _ = assign(x, centers)
    K = centers.shape[0]
    nk, s1, s2, _ = G.moments(x, centers, one_hot(label, K))
    assert np.all(nk > 0)
    return G.m_step(x.shape[0], centers, nk, s1, s2, reg_covar)


def gmm_fit_from(x, p, reg_covar=1e-6, tol=1e-3, max_iter=100):
    """_gmm_ref.fit's loop from the parameters p."""
    N = x.shape[0]
    lower, converged, n_iter = -np.inf, False, 0
    for n_iter in range(1, max_iter + 1):
        prev = lower
        _, ln, resp = G.log_resp(x, p["means"], p["prec_chol"], p["log_coef"])
        nk, s1, s2, ll = G.moments(x, p["means"], resp, ln)
        lower = float(ll) / N
        p = G.m_step(N, p["means"], nk, s1, s2, reg_covar)
        if abs(lower - prev) < tol:
            converged = True
            break
    p = dict(p)
    p.update(converged=converged, n_iter=n_iter, lower_bound=lower)
    return p


# ---- NDB ----------------------------------------------------------------------------------------------------------
def ndb(count_real, count_fake, alpha=0.05):
    """-> dict(ndb, ndb_over_k, js_divergence, bins, p_values, z) from two K-length histograms, bin by bin."""
    K = len(count_real)
    n, m = float(sum(count_real)), float(sum(count_fake))
    z, pv, bins = np.zeros(K), np.ones(K), np.zeros(K, bool)
    js = 0.0
    for k in range(K):
        P, Q = count_real[k] / n, count_fake[k] / m
        p = (n * P + m * Q) / (n + m)
        se = math.sqrt(p * (1.0 - p) * (1.0 / n + 1.0 / m))
        z[k] = (P - Q) / se if se > 0 else 0.0
        pv[k] = math.erfc(abs(z[k]) / math.sqrt(2.0))
        bins[k] = pv[k] < alpha
        M = 0.5 * (P + Q)
        js += (0.5 * P * math.log(P / M) if P > 0 else 0.0) + (0.5 * Q * math.log(Q / M) if Q > 0 else 0.0)
    return dict(ndb=int(bins.sum()), ndb_over_k=bins.sum() / K, js_divergence=js, bins=bins, p_values=pv, z=z)


# ---- shared inputs ------------------------------------------------------------------------------------------------
# (N, D, K) of the Lloyd comparisons against scikit-learn (tests/test_kmeans_cpu.py) and, the first two, of the device fit
FIT_CASES = ((300, 5, 4), (1000, 20, 10), (4099, 100, 17), (3000, 33, 64))
# (N, D, K, strided) of the exact assign / update cases on the device; tests/test_kmeans_cpu.py holds them against
# vg_kmeans_plan: every rows-per-workgroup and wave-split choice, one and several cluster chunks, one and several splits
EXACT_CASES = ((1, 1, 1, False), (63, 3, 2, True), (64, 4, 15, False), (65, 5, 16, True), (4099, 16, 17, False),
               (65, 17, 64, True), (63, 100, 65, False), (64, 100, 257, True), (65, 256, 1024, False), (4099, 100, 10, True),
               (63, 256, 2, False), (1, 5, 17, False))


def make_blobs(N, D, K, seed=0):
    """f32 [N, D]: unit noise around K centres ~ N(0, 3^2) -> (x, the true labels)."""
    r = np.random.default_rng(1000 * seed + N + 7 * D + 13 * K)
    cen = r.normal(size=(K, D)) * 3.0
    lab = r.integers(0, K, N)
    return (cen[lab] + r.normal(size=(N, D))).astype(np.float32), lab


def init_rows(N, K, seed=3):
    """K distinct row numbers.  Seed 3: of the seeds 0 .. 5 the first from which no cluster empties at any of FIT_CASES
    (random rows of a 64-blob mixture often put two centres into one blob and starve a third); the tests assert that
    condition on the reference before they compare anything."""
    return np.random.default_rng(seed).choice(N, K, replace=False)


def exact_inputs(N, D, K, seed=0):
    """Integer x with |.| <= 3 (a few rows at quarter-integers: the exact midpoint of two centres) and half-integer centres
    with |.| <= 3: every product, h and every sum is a multiple of 1/16 far below 2^53, exact in f64 in any order.  Where
    K >= 2 the LAST centre duplicates centre 0 (an exact tie at every row that centre 0 wins), and where K >= 3 row 0 is
    the midpoint of centres 0 and 1."""
    r = np.random.default_rng(5000 * seed + 7 * N + 3 * D + K)
    x = r.integers(-3, 4, (N, D)).astype(np.float32)
    c = r.integers(-6, 7, (K, D)) / 2.0
    if K >= 2:
        c[K - 1] = c[0]
    if K >= 3:
        x[0] = ((c[0] + c[1]) / 2.0).astype(np.float32)
    return x, c
