"""GPU: the k-means entry points (include/vaegan_hip.h, "K-means") against tests/_kmeans_ref.py.  Exact inputs (small
integers and half-integers, held exact on the CPU by tests/test_kmeans_cpu.py) are compared bit for bit over every branch
of the launch plan; random inputs within bounds counted from the roundings; then cluster.KMeans, the k-means start of the
mixture prior and the NDB metric against their restatements.  Outputs are NaN- or sentinel-filled first where the raw
entry point is called, so an element the kernel did not write shows."""
import io
from importlib import import_module

import numpy as np
import pytest
import torch

import _gmm_ref as G
import _kmeans_ref as R
import vaegan_amd as V
from test_gpu_parity import build

pytestmark = pytest.mark.gpu
DEV = "cuda"
PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
ops = import_module(PKG + ".ops")
L = import_module(PKG + "._lib")
latent = import_module(PKG + ".latent")
metrics = import_module(PKG + ".metrics")
U = 2.0 ** -53


def dev64(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(DEV)


def dev32(a, view=False, pad=7):
    """x on the device; view: rows further apart than D, the gaps NaN (never read)."""
    t = torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(DEV)
    if not view:
        return t
    big = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), dtype=torch.float32, device=DEV)
    big[:, :t.shape[1]] = t
    return big[:, :t.shape[1]]


def same_bits(got, want):
    return np.array_equal(got.cpu().numpy().view(np.int64), np.asarray(want, dtype=np.float64).view(np.int64))


def raw_assign(x, c, prev=None):
    """vg_kmeans_assign into NaN- / sentinel-filled outputs -> (label, dist2, resp, changed)."""
    N, D = x.shape
    K = c.shape[0]
    label = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    dist2 = torch.full((N,), float("nan"), dtype=torch.float64, device=DEV)
    resp = torch.full((N, K), float("nan"), dtype=torch.float64, device=DEV)
    changed = torch.full((1,), -7, dtype=torch.int32, device=DEV) if prev is not None else None
    stride = x.stride(0) if N > 1 else D
    L.check(L.load().vg_kmeans_assign(x.data_ptr(), N, D, stride, K, c.data_ptr(), label.data_ptr(), dist2.data_ptr(),
                                      resp.data_ptr(), L.ptr(prev), L.ptr(changed), L.stream_ptr()), "vg_kmeans_assign")
    return label, dist2, resp, changed


# ---- assign -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,K,view", R.EXACT_CASES)
def test_assign_is_exact_on_exact_inputs(N, D, K, view):
    x, c = R.exact_inputs(N, D, K)
    if N > 2:
        x[N // 2, D // 2] = np.nan                                      # a NaN row: label 0, NaN dist2
    want_label, want_d2, _ = R.assign(x, c)
    r = np.random.default_rng(N + K)
    prev = want_label.copy()
    flip = r.random(N) < 0.3
    prev[flip] = (prev[flip] + 1 + r.integers(0, 3, flip.sum())).astype(np.int32)          # differs, may exceed K - 1
    label, dist2, resp, changed = raw_assign(dev32(x, view), dev64(c), torch.as_tensor(prev).to(DEV))
    assert np.array_equal(label.cpu().numpy(), want_label)
    if N > 2:
        assert want_label[N // 2] == 0 and np.isnan(dist2[N // 2].item())
    assert np.array_equal(np.isnan(dist2.cpu().numpy()), np.isnan(want_d2))
    ok = ~np.isnan(want_d2)
    assert same_bits(dist2[torch.as_tensor(ok).to(DEV)], want_d2[ok])
    assert same_bits(resp, R.one_hot(want_label, K))
    assert int(changed.item()) == int(flip.sum())
    if K >= 2:
        assert not np.any(want_label == K - 1)                           # the duplicate of centre 0 never wins


@pytest.mark.parametrize("N,D,K", [(257, 5, 3), (1000, 17, 50), (300, 100, 200), (130, 256, 70)])
def test_assign_on_random_inputs_follows_the_restatement(N, D, K):
    r = np.random.default_rng(N + D + K)
    x = r.normal(size=(N, D)).astype(np.float32)
    c = r.normal(size=(K, D))
    want_label, want_d2, gap = R.assign(x, c)
    # a score is a sum of D + 1 terms (h and the products), each rounded once and added once, h itself a sum of D rounded
    # squares: |error| <= (2 D + 4) u (0.5 |c|^2 + sum |x_i| |c_i|) for the kernel and as much for the restatement.  The
    # inputs keep every best-to-second gap above the two together, so the labels must be equal.
    bound = 2 * (2 * D + 4) * U * R.score_scale(x, c).max()
    print("assign", (N, D, K), "smallest gap", gap.min(), "rounding bound", bound)
    assert gap.min() > bound
    label, dist2, _, _ = ops.kmeans_assign(dev32(x), dev64(c), want_dist2=True)
    assert np.array_equal(label.cpu().numpy(), want_label)
    # dist2: D differences rounded once, D squares and D additions: (2 D + 2) u dist2 each side
    err = np.abs(dist2.cpu().numpy() - want_d2)
    assert np.all(err <= 2 * (2 * D + 2) * U * want_d2)
    again = ops.kmeans_assign(dev32(x), dev64(c), want_dist2=True)
    assert torch.equal(again[0], label) and same_bits(again[1], dist2.cpu().numpy())


def test_assign_optional_outputs_and_the_op_wrapper():
    x, c = R.exact_inputs(65, 5, 16)
    xd, cd = dev32(x), dev64(c)
    want, _, _ = R.assign(x, c)
    label, d2, resp, chg = ops.kmeans_assign(xd, cd)
    assert d2 is None and resp is None and chg is None and np.array_equal(label.cpu().numpy(), want)
    label, d2, resp, chg = ops.kmeans_assign(xd, cd, want_label=False, prev_label=torch.as_tensor(want).to(DEV))
    assert label is None and d2 is None and resp is None and int(chg.item()) == 0
    with pytest.raises(RuntimeError, match="at least one output"):
        ops.kmeans_assign(xd, cd, want_label=False)
    with pytest.raises(RuntimeError, match="center"):
        ops.kmeans_assign(xd, cd.float())
    with pytest.raises(RuntimeError, match="1 <= K"):
        ops.kmeans_assign(xd, torch.zeros(1025, 5, dtype=torch.float64, device=DEV))


# ---- update -------------------------------------------------------------------------------------------------------
def raw_update(x, label, K, old, dist2, want=("sum", "center", "stats")):
    N, D = x.shape
    lib = L.load()
    nbytes = lib.vg_kmeans_update_ws_bytes(N, D, K)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV)
    count = torch.full((K,), -7, dtype=torch.int64, device=DEV)
    sm = torch.full((K, D), float("nan"), dtype=torch.float64, device=DEV) if "sum" in want else None
    center = torch.full((K, D), float("nan"), dtype=torch.float64, device=DEV) if "center" in want else None
    stats = torch.full((2,), float("nan"), dtype=torch.float64, device=DEV) if "stats" in want else None
    stride = x.stride(0) if N > 1 else D
    L.check(lib.vg_kmeans_update(x.data_ptr(), N, D, stride, K, label.data_ptr(), L.ptr(dist2), L.ptr(old),
                                 count.data_ptr(), L.ptr(sm), L.ptr(center), L.ptr(stats), ws.data_ptr(), nbytes,
                                 L.stream_ptr()), "vg_kmeans_update")
    return count, sm, center, stats


@pytest.mark.parametrize("N,D,K,view", R.EXACT_CASES)
def test_update_is_exact_on_integer_inputs(N, D, K, view):
    x, c = R.exact_inputs(N, D, K)
    x = np.round(x)                                                     # integers: sums and counts exact, one division
    label, d2, _ = R.assign(x, c)
    label = label.copy()
    if N > 4:
        label[1], label[N - 1] = -1, K                                  # masked rows: skipped
    d2 = np.round(d2 * 16) / 16
    count, s, center, stats = R.update(x, label, K, old=c, dist2=d2)
    g_count, g_sum, g_center, g_stats = raw_update(dev32(x, view), torch.as_tensor(label).to(DEV), K, dev64(c), dev64(d2))
    assert np.array_equal(g_count.cpu().numpy(), count) and count.sum() == N - (2 if N > 4 else 0)
    assert same_bits(g_sum, s) and same_bits(g_center, center)
    if K >= 2:
        assert count[K - 1] == 0                                         # the duplicate centre owns no row: it keeps `old`
    assert same_bits(g_center[torch.as_tensor(count == 0).to(DEV)], c[count == 0])
    assert g_stats[1].item() == d2.sum()                                 # sixteenths: exact in any order
    # stats[0]: K D squares of differences rounded once (the centre's division too), summed: (K D + 3) u of the sum
    assert abs(g_stats[0].item() - stats[0]) <= (K * D + 3) * 2 * U * stats[0]


def test_update_modes_one_cluster_and_count_only():
    x, _ = R.exact_inputs(4099, 16, 17)
    xd = dev32(x)
    one = torch.full((4099,), 5, dtype=torch.int32, device=DEV)         # every row in one cluster
    old = dev64(np.full((17, 16), 9.0))
    count, sm, center, stats = raw_update(xd, one, 17, old, None)
    assert count.tolist() == [4099 if k == 5 else 0 for k in range(17)]
    col = x.astype(np.float64).sum(axis=0)
    assert same_bits(sm[5], col) and same_bits(center[5], col / 4099.0)
    keep = [k for k in range(17) if k != 5]
    assert torch.all(center[keep] == 9.0) and torch.all(sm[keep] == 0.0) and stats[1].item() == 0.0
    count, sm, center, stats = raw_update(xd, one, 17, None, None, want=())                # count only: NDB's histogram
    assert count.tolist()[5] == 4099 and sm is None and center is None and stats is None
    count, _, _, _ = ops.kmeans_update(xd, one, 17)
    assert count.dtype == torch.int64 and int(count.sum().item()) == 4099


def test_update_on_random_inputs_is_repeatable_and_within_the_bound():
    N, D, K = 5000, 33, 70
    r = np.random.default_rng(5)
    x = r.normal(size=(N, D)).astype(np.float32)
    c = r.normal(size=(K, D))
    label, d2, _ = R.assign(x, c)
    count, s, center, stats = R.update(x, label, K, old=c, dist2=d2)
    a = raw_update(dev32(x), torch.as_tensor(label).to(DEV), K, dev64(c), dev64(d2))
    b = raw_update(dev32(x), torch.as_tensor(label).to(DEV), K, dev64(c), dev64(d2))
    for p, q in zip(a, b):
        assert torch.equal(p, q) if p.dtype == torch.int64 else same_bits(p, q.cpu().numpy())
    assert np.array_equal(a[0].cpu().numpy(), count)
    sabs = np.zeros((K, D))
    np.add.at(sabs, label, np.abs(x.astype(np.float64)))
    assert np.all(np.abs(a[1].cpu().numpy() - s) <= 2 * count.max() * U * sabs)           # n - 1 additions each side
    assert np.abs(a[2].cpu().numpy() - center).max() <= 2 * (count.max() + 1) * U * np.abs(x).max()
    assert abs(a[3][1].item() - stats[1]) <= 2 * N * U * stats[1]
    assert abs(a[3][0].item() - stats[0]) <= 1e-12 * stats[0]            # the centres' 1e-13 relative error, squared sums


# ---- seed ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,K", R.FIT_CASES[:3])
def test_seed_with_injected_draws_picks_the_restated_rows(N, D, K):
    x, _ = R.make_blobs(N, D, K)
    u = np.random.default_rng(N + K).random(K)                          # the inputs tests/test_kmeans_cpu.py holds safe
    idx, center, mind2, gap = R.seed(x, K, u)
    assert gap > 1e-8
    g_idx, g_center, g_mind2 = ops.kmeans_seed(dev32(x, True), K, u=dev64(u))
    assert np.array_equal(g_idx.cpu().numpy(), idx) and same_bits(g_center, center)
    assert np.abs(g_mind2.cpu().numpy() - mind2).max() <= 2 * (2 * D + 2) * U * mind2.max()


def test_seed_mind2_is_exact_on_integer_inputs_and_the_draws_are_the_materialised_ones():
    x, _ = R.exact_inputs(4099, 16, 17)
    x = np.round(x)
    u = np.random.default_rng(1).random(9)
    u[0] = 1.0 - 2.0 ** -53                                             # the clamp of idx[0]
    idx, center, mind2, _ = R.seed(x, 9, u)
    g_idx, g_center, g_mind2 = ops.kmeans_seed(dev32(x), 9, u=dev64(u))
    assert idx[0] == 4098 and np.array_equal(g_idx.cpu().numpy(), idx)
    assert same_bits(g_mind2, mind2) and same_bits(g_center, center)
    state = torch.tensor([11, 5], dtype=torch.int64, device=DEV)
    drawn = ops.rand_u01(9, state, ops.DRAW_KMEANS_U).double()
    a = ops.kmeans_seed(dev32(x), 9, state=state)
    b = ops.kmeans_seed(dev32(x), 9, u=drawn)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    one = ops.kmeans_seed(dev32(x), 1, u=dev64([0.5]))                   # K = 1: one launch
    assert one[0].tolist() == [2049] and same_bits(one[2], ((x - x[2049]) ** 2).sum(axis=1))


def test_fewer_distinct_rows_than_clusters_is_refused():
    same = np.repeat(R.exact_inputs(3, 4, 2)[0][:2], 20, axis=0)        # 40 rows, 2 distinct
    idx, center, mind2 = ops.kmeans_seed(dev32(same), 3, u=dev64([0.3, 0.5, 0.7]))
    assert torch.all(mind2 == 0) and np.unique(center.cpu().numpy(), axis=0).shape[0] == 2
    with pytest.raises(RuntimeError, match="duplicate seed rows"):
        V.KMeans.fit(dev32(same), 3, u=dev64([0.3, 0.5, 0.7]))
    bad = same.copy()
    bad[7, 1] = np.nan
    with pytest.raises(RuntimeError, match="not finite"):
        V.KMeans.fit(dev32(bad), 2, init=[0, 39])


# ---- fit ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted():
    """(x, device x, restated Lloyd, device KMeans) at (1000, 20, 10) from the same rows; shared, never modified."""
    N, D, K = R.FIT_CASES[1]
    x, _ = R.make_blobs(N, D, K)
    rows = R.init_rows(N, K)
    xd = dev32(x)
    return x, xd, R.lloyd(x, x[rows].astype(np.float64)), V.KMeans.fit(xd, K, init=rows)


def check_fit(ref, km, N, D, K):
    assert (km.n_iter_, km.converged, km.n_clusters, km.dim, km.n_fitted) == (ref["n_iter"], ref["converged"], K, D, N)
    assert np.array_equal(km.labels_.cpu().numpy(), ref["labels"])
    assert np.array_equal(km.counts_.cpu().numpy(), ref["counts"])
    assert np.abs(km.cluster_centers_.cpu().numpy() - ref["centers"]).max() <= 1e-12
    assert abs(km.inertia_ - ref["inertia"]) <= 1e-12 * ref["inertia"]
    assert km.cluster_centers_.dtype == torch.float64 and km.cluster_centers_.is_cuda


def test_fit_follows_the_restated_loop(fitted):
    x, xd, ref, km = fitted
    check_fit(ref, km, *R.FIT_CASES[1])
    N, D, K = R.FIT_CASES[0]
    x0, _ = R.make_blobs(N, D, K)
    c0 = x0[R.init_rows(N, K)].astype(np.float64)
    check_fit(R.lloyd(x0, c0), V.KMeans.fit(dev32(x0, True), K, init=dev64(c0)), N, D, K)  # centres given, strided rows
    capped = V.KMeans.fit(xd, 10, init=R.init_rows(1000, 10), max_iter=2)
    ref2 = R.lloyd(x, x[R.init_rows(1000, 10)].astype(np.float64), max_iter=2)
    assert not capped.converged and capped.n_iter_ == 2 and np.array_equal(capped.labels_.cpu().numpy(), ref2["labels"])
    assert abs(capped.inertia_ - ref2["inertia"]) <= 1e-12 * ref2["inertia"]


def test_kmeans_plus_plus_fit_predict_and_the_state_dict_round_trip(fitted):
    x, xd, ref, km = fitted
    assert torch.equal(km.predict(xd), km.labels_)
    pp = V.KMeans.fit(xd, 10, seed=4)
    again = V.KMeans.fit(xd, 10, seed=4)
    assert torch.equal(pp.cluster_centers_, again.cluster_centers_) and pp.inertia_ == again.inertia_
    assert pp.converged and int(pp.counts_.sum().item()) == 1000
    state = torch.tensor([4, 0], dtype=torch.int64, device=DEV)         # fit's generator state for seed=4
    start = float(ops.kmeans_seed(xd, 10, state=state)[2].sum().item())
    assert pp.inertia_ <= start                                         # Lloyd never raises the inertia of its start
    buf = io.BytesIO()
    torch.save(km.state_dict(), buf)
    buf.seek(0)
    sd = torch.load(buf, map_location="cpu")
    assert all(isinstance(v, torch.Tensor) for v in sd.values())
    back = V.KMeans.from_state_dict(sd)
    assert torch.equal(back.cluster_centers_, km.cluster_centers_) and torch.equal(back.counts_, km.counts_)
    assert (back.inertia_, back.n_iter_, back.converged, back.n_fitted) == (km.inertia_, km.n_iter_, km.converged, 1000)
    assert back.labels_ is None and torch.equal(back.predict(xd), km.labels_)
    assert torch.equal(pp.load_state_dict(sd).cluster_centers_, km.cluster_centers_)
    with pytest.raises(RuntimeError, match="20"):
        km.predict(xd[:, :5])


# ---- the mixture prior's k-means start ---------------------------------------------------------------------------
def parent_fit(x, K, idx, reg_covar=1e-6, tol=1e-3, max_iter=100):
    """GaussianMixturePrior.fit as it stood before the ``init`` keyword, from the public ops: what init="random" must
    still compute bit for bit."""
    N, D = x.shape
    rows = x[torch.as_tensor(idx, dtype=torch.int64, device=DEV)].double().contiguous()
    nk, s1, s2, _ = ops.gmm_moments(x, rows[:1].contiguous(), torch.ones(N, 1, dtype=torch.float64, device=DEV))
    nk0 = float(nk.item())
    delta = s1[0].cpu().numpy() / nk0
    prec = 1.0 / (np.diagonal(s2[0].cpu().numpy()) / nk0 - delta * delta + reg_covar)
    weights = np.full(K, 1.0 / K)
    means = rows.cpu().numpy()
    log_coef = np.log(weights) + np.log(np.sqrt(prec)).sum() - 0.5 * D * np.log(2.0 * np.pi)
    d_means, d_prec, d_coef = rows, dev64(np.tile(np.diag(np.sqrt(prec)), (K, 1, 1))), dev64(log_coef)
    lower, p = -np.inf, None
    for n_iter in range(1, max_iter + 1):
        prev = lower
        _, ln, resp = ops.gmm_log_resp(x, d_means, d_prec, d_coef)
        nk, s1, s2, ll = ops.gmm_moments(x, d_means, resp, ln)
        flat = torch.cat([ll, nk, s1.reshape(-1), s2.reshape(-1)]).cpu().numpy()
        lower = float(flat[0]) / N
        nk_h = flat[1:1 + K] + 10 * np.finfo(np.float64).eps
        weights = nk_h / N
        weights = weights / weights.sum()
        delta = flat[1 + K:1 + K + K * D].reshape(K, D) / nk_h[:, None]
        means = means + delta
        cov = flat[1 + K + K * D:].reshape(K, D, D) / nk_h[:, None, None] - delta[:, :, None] * delta[:, None, :]
        cov = 0.5 * (cov + cov.transpose(0, 2, 1))
        cov[:, np.arange(D), np.arange(D)] += reg_covar
        p = latent._gmm_host_step(weights, means, cov, reg_covar)
        d_means, d_prec, d_coef = dev64(p["means"]), dev64(p["prec_chol"]), dev64(p["log_coef"])
        if abs(lower - prev) < tol:
            break
    return p, n_iter, lower


def test_the_random_start_did_not_move():
    N, D, K = 2000, 8, 3
    xd = dev32(G.make_mixture(N, D, K))
    idx = G.default_init(N, K)
    p, n_iter, lower = parent_fit(xd, K, idx)
    for prior in (V.GaussianMixturePrior.fit(xd, K, init_idx=idx), V.GaussianMixturePrior.fit(xd, K, init="random", seed=0)):
        assert (prior.n_iter, prior.lower_bound) == (n_iter, lower)
        for k in ("weights", "means", "covariances", "prec_chol", "cov_chol", "cdf"):
            assert same_bits(getattr(prior, k), p[k]), k


@pytest.mark.parametrize("N,D,K", [(2000, 8, 4), (3000, 33, 5)])
def test_the_kmeans_start_follows_the_restatement(N, D, K):
    x, _ = R.make_blobs(N, D, K)
    xd = dev32(x)
    rows = R.init_rows(N, K)
    ref_km = R.lloyd(x, x[rows].astype(np.float64))
    assert not ref_km["emptied"] and ref_km["min_gap"] > 1e-8
    ref = R.gmm_fit_from(x, R.gmm_start(x, ref_km["centers"]))
    km = V.KMeans.fit(xd, K, init=rows)
    prior = V.GaussianMixturePrior.fit(xd, K, init=km)
    assert (prior.n_iter, prior.converged) == (ref["n_iter"], ref["converged"])
    dev = {k: G.rel_dev(getattr(prior, k).cpu().numpy(), ref[k])
           for k in ("weights", "means", "covariances", "prec_chol", "cov_chol", "cdf")}
    dev["lower_bound"] = abs(prior.lower_bound - ref["lower_bound"]) / abs(ref["lower_bound"])
    print("k-means start against the restatement", (N, D, K), dev, "iterations", prior.n_iter)
    for name, v in dev.items():
        assert v <= G.FIT_BOUND, (name, v)                               # the bound tests/test_gpu_gmm.py holds the device fit to
    auto = V.GaussianMixturePrior.fit(xd, K, init="kmeans", seed=2)      # k-means++ inside
    assert auto.converged and np.isfinite(auto.lower_bound) and auto.n_components == K
    with pytest.raises(RuntimeError, match="empty"):
        far = km.cluster_centers_.clone()
        far[0] = 1e6                                                    # a centre no row is nearest to
        V.GaussianMixturePrior.fit(xd, K, init=V.KMeans(far, km.counts_))


# ---- NDB ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ndb_sets():
    """Real and two fake feature sets from one 8-mode mixture: same distribution, and mode 3 dropped."""
    r = np.random.default_rng(21)
    D, M = 16, 8
    cen = r.normal(size=(M, D)) * 3.0
    def draw(n, modes):
        lab = modes[r.integers(0, len(modes), n)]
        return (cen[lab] + r.normal(size=(n, D))).astype(np.float32), lab
    real, real_lab = draw(6000, np.arange(M))
    same, _ = draw(6000, np.arange(M))
    dropped, _ = draw(6000, np.array([m for m in range(M) if m != 3]))
    return real, real_lab, same, dropped


def test_ndb_follows_the_restatement_and_flags_a_dropped_mode(ndb_sets):
    real, real_lab, same, dropped = ndb_sets
    K, alpha = 24, 0.05
    rd = dev32(real)
    out = V.ndb(rd, dev32(same), n_bins=K, alpha=alpha, seed=1)
    km = out["kmeans"]
    centres = km.cluster_centers_.cpu().numpy()
    ref_real = np.bincount(R.assign(real, centres)[0], minlength=K)
    ref_fake = np.bincount(R.assign(same, centres)[0], minlength=K)
    assert np.array_equal(km.counts_.cpu().numpy(), ref_real)
    want = R.ndb(ref_real, ref_fake, alpha)
    assert out["ndb"] == want["ndb"] and np.array_equal(out["bins"], want["bins"])
    assert abs(out["js_divergence"] - want["js_divergence"]) <= 1e-15 and out["ndb_over_k"] == want["ndb"] / K
    assert np.array_equal(out["real_proportions"], ref_real / 6000) and np.array_equal(out["fake_proportions"], ref_fake / 6000)
    # identically distributed: each bin is flagged with probability ~alpha; mean alpha K = 1.2, and 6 is more than four
    # standard deviations (sqrt(K alpha (1 - alpha)) = 1.07) above it
    assert out["ndb"] <= alpha * K + 5
    drop = metrics.ndb(None, dev32(dropped), alpha=alpha, kmeans=km)      # the real side is clustered once
    assert drop["kmeans"] is km
    bin_mode = np.array([np.bincount(real_lab[R.assign(real, centres)[0] == k], minlength=8).argmax() for k in range(K)])
    mode3 = bin_mode == 3
    assert mode3.any() and np.all(drop["bins"][mode3]) and np.all(drop["fake_proportions"][mode3] < 0.002)
    assert drop["ndb"] > out["ndb"] and drop["js_divergence"] > 10 * out["js_divergence"]
    assert V.ndb(rd, rd, n_bins=K, seed=1)["ndb"] == 0


class Capture:
    """A feature_fn that keeps what it returned: real and fake features of each batch, in turn."""

    def __init__(self, fn):
        self.fn, self.out = fn, []

    def __call__(self, u8):
        f = self.fn(u8)
        self.out.append(f.clone())
        return f


def test_evaluate_generation_ndb_equals_the_loop_from_public_pieces():
    e, g, _, _ = build(64, "fp32")
    fn = V.encoder_features(e)
    gen = torch.Generator().manual_seed(5)
    vl = [(torch.rand(8, 3, 64, 64, generator=gen) * 2 - 1).to(DEV) for _ in range(3)]
    zs = [torch.randn(8, 100, generator=gen).to(DEV) for _ in vl]
    base = V.evaluate_generation(g, vl, noise_fn=lambda i, b: zs[i], feature_fn=fn)
    assert set(base) == {"ssim", "samples", "batches", "fid", "feature_dim", "precision", "recall", "f1"}      # today's keys
    cap = Capture(fn)
    got = V.evaluate_generation_ndb(g, vl, ndb_bins=4, ndb_seed=2, noise_fn=lambda i, b: zs[i], feature_fn=cap)
    assert set(got) == set(base) | {"ndb", "ndb_over_k", "js_divergence"}
    assert all(got[k] == base[k] for k in base)
    want = V.ndb(torch.cat(cap.out[0::2]), torch.cat(cap.out[1::2]), n_bins=4, seed=2)
    assert (got["ndb"], got["ndb_over_k"], got["js_divergence"]) == (want["ndb"], want["ndb_over_k"], want["js_divergence"])
    with pytest.raises(RuntimeError, match="feature_fn"):
        V.evaluate_generation_ndb(g, vl, ndb_bins=4)
