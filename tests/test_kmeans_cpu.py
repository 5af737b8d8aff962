"""CPU: k-means before any kernel runs.  (1) tests/_kmeans_ref.py's Lloyd loop -- the loop cluster.KMeans.fit runs --
against scikit-learn's KMeans from the same centres, with the conditions on the inputs that make exact label and index
comparison safe; (2) the seeding's properties; (3) the k-means start of the mixture prior against plain numpy and
scikit-learn's GaussianMixture; (4) the NDB arithmetic against scipy; (5) the exact-input tables of the GPU tests are exact
in f64 (held against integer / Fraction arithmetic); (6) the C ABI declarations, the ctypes table, host-side argument
validation, the package exports, the "no CPU path" errors and the launch plan's coverage by the GPU case table."""
import ctypes
import inspect
import os
import re
from fractions import Fraction
from importlib import import_module

import numpy as np
import pytest
import torch
from scipy.spatial.distance import jensenshannon
from scipy.stats import norm
from sklearn.cluster import KMeans as SkKMeans
from sklearn.mixture import GaussianMixture

import _gmm_ref as G
import _kmeans_ref as R

PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vg_kmeans_plan", "vg_kmeans_assign", "vg_kmeans_update_ws_bytes", "vg_kmeans_update", "vg_kmeans_seed_ws_bytes",
       "vg_kmeans_seed")
GAP = 1e-8                                                               # f64 rounding of a score or a cumulative sum: ~1e-11


# ---- 1. the restated Lloyd loop against scikit-learn ----------------------------------------------------------------
@pytest.mark.parametrize("N,D,K", R.FIT_CASES)
def test_restated_lloyd_follows_scikit_learn(N, D, K):
    x, _ = R.make_blobs(N, D, K)
    c0 = x[R.init_rows(N, K)].astype(np.float64)
    p = R.lloyd(x, c0)
    # conditions on the INPUTS, asserted on the reference alone: no cluster empties (scikit-learn would relocate it) and
    # no row sits within rounding of two centres, so labels can be compared exactly
    assert not p["emptied"] and np.all(p["counts"] > 0)
    assert p["min_gap"] > GAP, p["min_gap"]
    sk = SkKMeans(n_clusters=K, init=c0, n_init=1, algorithm="lloyd", tol=1e-4).fit(x.astype(np.float64))
    print("lloyd vs scikit-learn", (N, D, K), "iterations", p["n_iter"], "centre error",
          np.abs(p["centers"] - sk.cluster_centers_).max(), "min gap", p["min_gap"])
    assert p["n_iter"] == sk.n_iter_ and p["converged"]
    assert np.array_equal(p["labels"], sk.labels_)
    assert np.abs(p["centers"] - sk.cluster_centers_).max() <= 1e-12
    assert abs(p["inertia"] - sk.inertia_) <= 1e-12 * sk.inertia_


# ---- 2. seeding ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,K", R.FIT_CASES)
def test_seeding_properties_and_safe_gaps(N, D, K):
    x, _ = R.make_blobs(N, D, K)
    u = np.random.default_rng(N + K).random(K)
    idx, center, mind2, gap = R.seed(x, K, u)
    assert len(set(idx.tolist())) == K                                  # a picked row has mind2 > 0: never a chosen one
    assert idx[0] == min(int(u[0] * N), N - 1)
    assert gap > GAP, gap                                               # condition on the inputs for exact idx comparison
    assert np.array_equal(center, x[idx].astype(np.float64))
    d = ((x.astype(np.float64)[:, None, :] - center[None]) ** 2).sum(axis=2).min(axis=1)
    assert np.allclose(mind2, d, rtol=1e-12, atol=0) and np.all(mind2[idx] == 0)


def test_seeding_clamps_and_handles_a_zero_total():
    x, _ = R.make_blobs(300, 5, 4)
    u = np.array([1.0 - 2.0 ** -53, 1.0 - 2.0 ** -53, 0.0, 0.5])
    idx, _, _, _ = R.seed(x, 4, u)
    assert idx[0] == 299                                                # (int64)(u N) = N - 1 at the top of [0, 1)
    assert idx[2] == 0 if idx[0] != 0 and idx[1] != 0 else True         # u = 0: the first row with mind2 > 0
    same = np.repeat(x[:1], 10, axis=0)                                 # fewer than K distinct rows: total = 0 from step 1
    idx, center, mind2, _ = R.seed(same, 3, np.array([0.3, 0.5, 0.7]))
    assert idx.tolist() == [3, 9, 9] and np.all(mind2 == 0)             # nothing exceeds 0: clamped to N - 1; duplicates
    assert np.unique(center, axis=0).shape[0] == 1


# ---- 3. the k-means start of the mixture prior --------------------------------------------------------------------
@pytest.mark.parametrize("N,D,K", [(600, 5, 3), (2000, 8, 4)])
def test_gmm_start_is_the_m_step_on_one_hot_responsibilities(N, D, K):
    x, _ = R.make_blobs(N, D, K)
    km = R.lloyd(x, x[R.init_rows(N, K)].astype(np.float64))
    p0 = R.gmm_start(x, km["centers"], 1e-6)
    x64 = x.astype(np.float64)
    for k in range(K):
        rows = x64[km["labels"] == k]
        assert np.allclose(p0["means"][k], rows.mean(axis=0), rtol=0, atol=1e-12)
        want = np.cov(rows.T, bias=True).reshape(D, D) + 1e-6 * np.eye(D)
        assert np.allclose(p0["covariances"][k], want, rtol=0, atol=1e-11)
        assert abs(p0["weights"][k] - len(rows) / N) < 1e-14
    p = R.gmm_fit_from(x, p0)
    prec = np.stack([u @ u.T for u in p0["prec_chol"]])
    g = GaussianMixture(K, covariance_type="full", weights_init=p0["weights"] / p0["weights"].sum(), means_init=p0["means"],
                        precisions_init=prec, reg_covar=1e-6, tol=1e-3, max_iter=100).fit(x64)
    assert (p["n_iter"], p["converged"]) == (g.n_iter_, g.converged_)
    for name, ref in (("weights", g.weights_), ("means", g.means_), ("prec_chol", g.precisions_cholesky_)):
        assert G.rel_dev(p[name], ref) <= G.FIT_BOUND, name
    assert abs(p["lower_bound"] - g.lower_bound_) <= G.FIT_BOUND * abs(g.lower_bound_)


# ---- 4. NDB -------------------------------------------------------------------------------------------------------
def test_ndb_arithmetic_against_scipy():
    M = import_module(PKG + ".metrics")
    r = np.random.default_rng(3)
    cr = r.integers(0, 200, 40)
    cf = r.integers(0, 200, 40)
    cr[5] = cf[5] = 0                                                   # se = 0: an empty bin on both sides
    cr[6], cf[7] = 0, 0                                                 # a bin empty on one side each
    for got in (M.ndb_statistics(cr, cf, 0.05), R.ndb(cr, cf, 0.05)):
        n, m = cr.sum(), cf.sum()
        P, Q = cr / n, cf / m
        pooled = (cr + cf) / (n + m)
        se = np.sqrt(pooled * (1 - pooled) * (1 / n + 1 / m))
        z = np.where(se > 0, (P - Q) / np.where(se > 0, se, 1.0), 0.0)
        pv = 2.0 * norm.cdf(-np.abs(z))
        assert np.allclose(got["z"], z, rtol=1e-12, atol=1e-14) and got["z"][5] == 0.0 and got["p_values"][5] == 1.0
        assert np.allclose(got["p_values"], pv, rtol=1e-10, atol=1e-300)
        assert np.array_equal(got["bins"], pv < 0.05) and got["ndb"] == int((pv < 0.05).sum())
        assert abs(got["ndb_over_k"] - got["ndb"] / 40) < 1e-15
        assert abs(got["js_divergence"] - jensenshannon(P, Q) ** 2) < 1e-14
    same = M.ndb_statistics(cr, cr * 3)                                 # identical proportions
    assert same["ndb"] == 0 and same["js_divergence"] == 0.0 and not same["bins"].any()
    one = M.ndb_statistics([10], [7])                                   # K = 1: p = 1, se = 0
    assert one["ndb"] == 0 and one["z"][0] == 0.0
    with pytest.raises(ValueError):
        M.ndb_statistics([1, 2], [0, 0])


# ---- 5. the exact-input tables are exact ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,K", [(63, 3, 2), (65, 17, 64), (64, 100, 257), (65, 256, 1024)])
def test_exact_assign_table_is_exact_in_f64_and_its_ties_are_ties(N, D, K):
    x, c = R.exact_inputs(N, D, K)
    x4 = np.round(x.astype(np.float64) * 4).astype(np.int64)            # x in quarters
    c2 = np.round(c * 2).astype(np.int64)                               # centres in halves
    assert np.array_equal(x4 / 4.0, x.astype(np.float64)) and np.array_equal(c2 / 2.0, c)
    s8 = (c2 * c2).sum(axis=1)[None, :] - x4 @ c2.T                     # 8 s, integers
    assert np.abs(s8).max() < 2 ** 40
    s = R.scores(x, c)
    for n in range(0, N, 7):
        for k in range(0, K, max(1, K // 9)):
            assert Fraction(float(s[n, k])) == Fraction(int(s8[n, k]), 8)
    label, dist2, _ = R.assign(x, c)
    assert np.array_equal(label, np.argmin(s8, axis=1))
    d4 = x4 - 2 * c2[label]
    assert np.array_equal(dist2 * 16, (d4 * d4).sum(axis=1))
    if K >= 2:
        assert np.array_equal(s8[:, 0], s8[:, K - 1]) and not np.any(label == K - 1)       # the duplicate never wins
    if K >= 3:
        assert s8[0, 0] == s8[0, 1]                                      # the midpoint row is equidistant


@pytest.mark.parametrize("N,D,K", [(63, 3, 2), (4099, 16, 17), (65, 256, 1024)])
def test_exact_update_table_is_exact_in_f64(N, D, K):
    x, c = R.exact_inputs(N, D, K)
    label, _, _ = R.assign(x, c)
    count, s, center, _ = R.update(x, label, K, old=c)
    x4 = np.round(x.astype(np.float64) * 4).astype(np.int64)
    for k in range(K):
        rows = x4[label == k]
        assert count[k] == len(rows) and np.array_equal(s[k] * 4, rows.sum(axis=0))
        want = c[k] if len(rows) == 0 else s[k] / float(len(rows))
        assert np.array_equal(center[k], want)
    assert count.sum() == N


# ---- 6. the library, host side --------------------------------------------------------------------------------------
def test_header_declares_and_binding_table_binds_the_new_entry_points():
    L = import_module(PKG + "._lib")
    src = open(os.path.join(ROOT, "include", "vaegan_hip.h")).read()
    lib = L.load()
    for name in NEW:
        assert re.search(r"\b(int|int64_t)\s+" + name + r"\s*\(", src), name
        assert name in L.SIGNATURES, name
        assert hasattr(lib, name), name
    m = re.search(r"#define\s+VG_ABI_VERSION\s+(\d+)", src)
    assert int(m.group(1)) == L.ABI_VERSION >= 30 and lib.vg_abi_version() == L.ABI_VERSION
    ops = import_module(PKG + ".ops")
    assert int(re.search(r"#define\s+VG_DRAW_KMEANS_U\s+(\d+)", src).group(1)) == ops.DRAW_KMEANS_U == 42
    for text in ("K-means", "LOWEST k", "two-level", "vg_km_plan"):
        assert text in src
    assert "kmeans.hip" in open(os.path.join(ROOT, PKG, "csrc", "Makefile")).read()


def test_c_abi_of_the_kmeans_entry_points_rejects_bad_arguments_on_host():
    L = import_module(PKG + "._lib")
    lib = L.load()
    b = ctypes.c_void_p(256)                                             # never dereferenced: validation comes first
    odd = ctypes.c_void_p(260)
    big = 1 << 40
    shapes = ((0, 8, 3), (1 << 31, 8, 3), (10, 0, 3), (10, 257, 3), (10, 8, 0), (10, 8, 1025))
    for q in (lib.vg_kmeans_update_ws_bytes, lib.vg_kmeans_seed_ws_bytes):
        assert q(200000, 100, 200) > 0 and q(2 ** 31 - 1, 256, 1024) > 0 and q(1, 1, 1) > 0
        for bad in shapes:
            assert q(*bad) == -1, bad
    plan = L.KMPlan()
    assert lib.vg_kmeans_plan(10, 8, 3, ctypes.byref(plan)) == 0
    assert lib.vg_kmeans_plan(10, 8, 3, None) == -1
    for bad in shapes:
        assert lib.vg_kmeans_plan(*bad, ctypes.byref(plan)) == -1, bad
    lim = dict(N=0), dict(N=1 << 31), dict(D=0), dict(D=257, stride=257), dict(K=0), dict(K=1025), dict(stride=7)
    # vg_kmeans_assign(x, N, D, stride, K, center, label, dist2, resp, prev_label, changed, stream)
    def a(x=b, N=10, D=8, stride=8, K=3, c=b, lab=b, d2=b, rs=b, prev=b, chg=b):
        return lib.vg_kmeans_assign(x, N, D, stride, K, c, lab, d2, rs, prev, chg, None)
    for kw in lim + (dict(x=None), dict(c=None), dict(lab=None, d2=None, rs=None, prev=None, chg=None),
                     dict(prev=None), dict(chg=None)):
        assert a(**kw) == -1, kw                                          # changed without prev_label and the reverse
    assert a(c=odd) == -2 and a(d2=odd) == -2 and a(rs=odd) == -2
    # vg_kmeans_update(x, N, D, stride, K, label, dist2, old, count, sum, center, stats, ws, ws_bytes, stream)
    def u(x=b, N=10, D=8, stride=8, K=3, lab=b, d2=b, old=b, cnt=b, sm=b, cen=b, st=b, ws=b, wsb=big):
        return lib.vg_kmeans_update(x, N, D, stride, K, lab, d2, old, cnt, sm, cen, st, ws, wsb, None)
    for kw in lim + (dict(x=None), dict(lab=None), dict(cnt=None), dict(ws=None), dict(old=None), dict(st=None),
                     dict(wsb=8), dict(wsb=lib.vg_kmeans_update_ws_bytes(10, 8, 3) - 1)):
        assert u(**kw) == -1, kw                                          # center without old; dist2 without stats
    for name in ("d2", "old", "cnt", "sm", "cen", "st", "ws"):
        assert u(**{name: odd}) == -2, name
    # vg_kmeans_seed(x, N, D, stride, K, u, rng, idx, center, ws, ws_bytes, stream)
    def s(x=b, N=10, D=8, stride=8, K=3, uu=b, rng=None, idx=b, cen=b, ws=b, wsb=big):
        return lib.vg_kmeans_seed(x, N, D, stride, K, uu, rng, idx, cen, ws, wsb, None)
    for kw in lim + (dict(x=None), dict(idx=None), dict(cen=None), dict(ws=None), dict(uu=None),
                     dict(wsb=lib.vg_kmeans_seed_ws_bytes(10, 8, 3) - 1)):
        assert s(**kw) == -1, kw                                          # no u and no generator
    for name in ("uu", "cen", "ws"):
        assert s(**{name: odd}) == -2, name
    assert s(uu=None, rng=odd) == -2


def test_package_exports_and_host_tensors_are_refused():
    import vaegan_amd as V
    C = import_module(PKG + ".cluster")
    M = import_module(PKG + ".metrics")
    for name in ("KMeans", "ndb", "cluster"):
        assert name in V.__all__ and hasattr(V, name) and name in V.__doc__, name
    assert V.KMeans is C.KMeans and V.ndb is M.ndb and V.cluster is C
    ops = import_module(PKG + ".ops")
    x = torch.randn(32, 4)
    c = torch.zeros(2, 4, dtype=torch.float64)
    for call in (lambda: ops.kmeans_assign(x, c), lambda: ops.kmeans_update(x, torch.zeros(32, dtype=torch.int32), 2),
                 lambda: ops.kmeans_seed(x, 2, u=torch.zeros(2, dtype=torch.float64)), lambda: V.KMeans.fit(x, 2),
                 lambda: V.KMeans(c, torch.zeros(2, dtype=torch.int64)), lambda: V.ndb(x, x, n_bins=2),
                 lambda: V.GaussianMixturePrior.fit(x, 2, init="kmeans")):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    p = ops.kmeans_plan(200000, 100, 200)                                # the plan needs no GPU
    assert p["update_ws_bytes"] == 8 * (p["update_splits"] * (200 * 100 + 200 + 1) + 200) < 32 << 20 and p["update_splits"] <= 128
    assert p["seed_block"] == R.SEED_BLOCK and p["seed_ws_bytes"] == 8 * (200000 + p["seed_blocks"])
    with pytest.raises(RuntimeError):
        ops.kmeans_plan(10, 257, 3)


def test_fit_validates_its_arguments_before_any_launch():
    import vaegan_amd as V

    class OnDevice:                                                      # fit looks at the description before any launch
        is_cuda, dtype, shape = True, torch.float32, (5, 4)

        def dim(self):
            return 2

    x = OnDevice()
    with pytest.raises(RuntimeError, match="cannot seed"):
        V.KMeans.fit(x, 6)
    for bad in (0, 1025):
        with pytest.raises(RuntimeError, match="n_clusters"):
            V.KMeans.fit(x, bad)
    for bad in ([0, 0, 1], [0, 1], [0, 1, 5], [-1, 0, 1], [0.0, 1.0, 2.0]):
        with pytest.raises(RuntimeError, match="duplicate seed rows|row numbers"):
            V.KMeans.fit(x, 3, init=bad)
    with pytest.raises(RuntimeError, match="k-means\\+\\+"):
        V.KMeans.fit(x, 3, init="random")
    with pytest.raises(RuntimeError, match="max_iter"):
        V.KMeans.fit(x, 3, max_iter=0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        V.KMeans.fit(x, 3, init=torch.zeros(3, 4, dtype=torch.float64))
    x.dtype = torch.float64
    with pytest.raises(RuntimeError, match="f32"):
        V.KMeans.fit(x, 3)
    x.dtype = torch.float32
    # GaussianMixturePrior.fit(init=)
    with pytest.raises(RuntimeError, match="init_idx"):
        V.GaussianMixturePrior.fit(x, 3, init="kmeans", init_idx=[0, 1, 2])
    with pytest.raises(RuntimeError, match="init must be"):
        V.GaussianMixturePrior.fit(x, 3, init="k-means++")
    km = V.KMeans.__new__(V.KMeans)
    km.n_clusters, km.dim = 2, 4
    with pytest.raises(RuntimeError, match="2 clusters"):
        V.GaussianMixturePrior.fit(x, 3, init=km)
    km.n_clusters, km.dim = 3, 7
    with pytest.raises(RuntimeError, match="7"):
        V.GaussianMixturePrior.fit(x, 3, init=km)


def test_new_keywords_default_to_what_was_there():
    import vaegan_amd as V
    sig = inspect.signature(V.GaussianMixturePrior.fit)
    assert list(sig.parameters)[-1] == "init" and sig.parameters["init"].default == "random"
    assert [(n, p.default) for n, p in inspect.signature(V.KMeans.fit).parameters.items()][1:] == [
        ("n_clusters", inspect.Parameter.empty), ("init", "k-means++"), ("max_iter", 300), ("tol", 1e-4), ("seed", 0),
        ("u", None)]
    assert [(n, p.default) for n, p in inspect.signature(V.ndb).parameters.items()][2:] == [
        ("n_bins", 100), ("alpha", 0.05), ("seed", 0), ("kmeans", None)]


# ---- 7. the GPU case table covers every branch of the launchers ---------------------------------------------------------
def test_exact_case_table_covers_the_launch_plan():
    ops = import_module(PKG + ".ops")
    plans = [ops.kmeans_plan(N, D, K) for N, D, K, _ in R.EXACT_CASES]
    assert {(p["assign_rows"], p["assign_row_split"]) for p in plans} == {(64, 1), (64, 0), (32, 0)}
    assert {p["assign_tile"] for p in plans} == {16}
    assert {p["update_chunks"] == 1 for p in plans} == {True, False}
    assert {p["update_splits"] == 1 for p in plans} == {True, False}
    assert {p["assign_grid"] == 1 for p in plans} == {True, False}
    assert {p["seed_blocks"] == 1 for p in plans} == {True, False}
    assert {s for _, _, _, s in R.EXACT_CASES} == {True, False}
    # the thresholds themselves
    assert ops.kmeans_plan(100, 224, 64)["assign_rows"] == 64 and ops.kmeans_plan(100, 225, 64)["assign_rows"] == 32
    assert ops.kmeans_plan(100, 8, 48)["assign_row_split"] == 1 and ops.kmeans_plan(100, 8, 49)["assign_row_split"] == 0
    for N, D, K, _ in R.EXACT_CASES + ((2 ** 31 - 1, 256, 1024, False), (200000, 100, 200, False)):
        p = ops.kmeans_plan(N, D, K)
        assert p["assign_lds_bytes"] <= 65536 and p["update_chunk"] * D * 8 <= 49152
        assert p["update_chunks"] == -(-K // p["update_chunk"]) and 1 <= p["update_splits"] <= 1024
        assert p["update_rows_per_split"] % 256 == 0 and p["update_splits"] * p["update_rows_per_split"] >= N
        assert (p["update_splits"] - 1) * p["update_rows_per_split"] < N
