"""CPU: the feature-space metrics without a GPU.  (1) the C ABI: version 14, the new declarations, the ctypes table, the
exports, host-side argument validation and the workspace condition of include/vaegan_hip.h ("Feature-space metrics");
(2) the f64 numpy restatement tests/_metrics_ref.py -- the yardstick of the GPU tests -- against closed forms, against
scipy.linalg.sqrtm and against sklearn.neighbors.NearestNeighbors; (3) metrics.frechet_distance fed host-made
FeatureStats state against the restatement; (4) the package surface and the loud failure off the GPU.
Parity with the torchmetrics package itself is unpinned: it is not installed."""
import ctypes
import os
import re
from importlib import import_module

import numpy as np
import pytest
import torch

import _metrics_ref as R

PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vg_feat_stats_accum_ws_bytes", "vg_feat_stats_accum", "vg_knn_radius2_ws_bytes", "vg_knn_radius2",
       "vg_manifold_cover_ws_bytes", "vg_manifold_cover")


# ---- 1: C ABI -------------------------------------------------------------------------------------------------------
def test_abi_14_declares_binds_and_exports_the_metric_entry_points():
    L = import_module(PKG + "._lib")
    src = open(os.path.join(ROOT, "include", "vaegan_hip.h")).read()
    m = re.search(r"#define\s+VG_ABI_VERSION\s+(\d+)", src)
    assert int(m.group(1)) == L.ABI_VERSION >= 14
    assert "Feature-space metrics" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = L.load()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert lib.vg_abi_version() == L.ABI_VERSION


def test_workspace_is_linear_in_the_rows_and_small_at_the_reference_sizes():
    """The N x N matrix is never written: the workspace is O((Nq + Nr) k splits), with at most 16 splits."""
    lib = import_module(PKG + "._lib").load()
    assert 0 < lib.vg_knn_radius2_ws_bytes(30000, 2048, 3) < 64 << 20
    assert 0 < lib.vg_manifold_cover_ws_bytes(30000, 30000, 2048) < 64 << 20
    for N in (2, 100, 3000, 30000, 1 << 20):
        for D in (1, 64, 2048):
            for k in (1, 3, 8):
                if k < N:
                    assert 0 < lib.vg_knn_radius2_ws_bytes(N, D, k) <= 4 * N * k * 16 + 4 * N + 256
            assert 0 < lib.vg_manifold_cover_ws_bytes(N, 2 * N, D) <= 4 * N * 16 + 4 * 3 * N + 512
            assert 0 < lib.vg_manifold_cover_ws_bytes(2 * N, N, D) <= 4 * 2 * N * 16 + 4 * 3 * N + 512
    # statistics: partial 64 x 64 tiles of the upper triangle per row split; independent of n once n is large
    assert lib.vg_feat_stats_accum_ws_bytes(0, 64) == 0
    assert 0 < lib.vg_feat_stats_accum_ws_bytes(30000, 2048) <= 18 << 20
    assert lib.vg_feat_stats_accum_ws_bytes(30000, 2048) == lib.vg_feat_stats_accum_ws_bytes(3000000, 2048)
    for D in (1, 37, 64, 100, 200, 2048):
        assert 0 < lib.vg_feat_stats_accum_ws_bytes(1 << 30, D) <= 18 << 20


def test_c_abi_of_the_metric_entry_points_rejects_bad_arguments_on_host():
    lib = import_module(PKG + "._lib").load()
    buf = ctypes.c_void_p(4096)                       # never dereferenced: every call below is rejected before a launch
    big = 1 << 40
    assert lib.vg_feat_stats_accum_ws_bytes(-1, 64) == -1
    assert lib.vg_feat_stats_accum_ws_bytes(10, 0) == -1 and lib.vg_feat_stats_accum_ws_bytes(10, 2049) == -1
    assert lib.vg_feat_stats_accum(buf, 10, 0, 4, buf, buf, buf, big, None) == -1
    assert lib.vg_feat_stats_accum(buf, 10, 4, 3, buf, buf, buf, big, None) == -1                    # row stride < D
    assert lib.vg_feat_stats_accum(buf, 10, 4, 4, None, buf, buf, big, None) == -1
    assert lib.vg_feat_stats_accum(buf, 10, 4, 4, buf, buf, buf, 8, None) == -1                      # workspace too small
    assert lib.vg_feat_stats_accum(buf, 10, 4, 4, ctypes.c_void_p(4100), buf, buf, big, None) == -2
    assert lib.vg_feat_stats_accum(None, 0, 4, 4, buf, buf, None, 0, None) == 0                      # n == 0: a no-op
    assert lib.vg_knn_radius2_ws_bytes(10, 4, 0) == -1 and lib.vg_knn_radius2_ws_bytes(10, 4, 9) == -1
    assert lib.vg_knn_radius2_ws_bytes(3, 4, 3) == -1                                                # k < N
    assert lib.vg_knn_radius2_ws_bytes(10, 0, 1) == -1 and lib.vg_knn_radius2_ws_bytes(10, 4096, 1) == -1
    assert lib.vg_knn_radius2(buf, 3, 4, 3, buf, buf, big, None) == -1
    assert lib.vg_knn_radius2(buf, 10, 4, 3, buf, buf, 8, None) == -1
    assert lib.vg_knn_radius2(None, 10, 4, 3, buf, buf, big, None) == -1
    assert lib.vg_knn_radius2(ctypes.c_void_p(4100), 10, 4, 3, buf, buf, big, None) == -2
    assert lib.vg_manifold_cover_ws_bytes(0, 10, 4) == -1 and lib.vg_manifold_cover_ws_bytes(10, 0, 4) == -1
    assert lib.vg_manifold_cover(buf, 10, buf, 10, 4, None, buf, buf, buf, big, None) == -1
    assert lib.vg_manifold_cover(buf, 10, buf, 10, 4, buf, buf, buf, buf, 8, None) == -1
    assert lib.vg_manifold_cover(buf, 10, buf, 10, 4, buf, buf, ctypes.c_void_p(4100), buf, big, None) == -2


# ---- 2: the restatement against closed forms and independent libraries ---------------------------------------------
def test_fid_restatement_closed_forms():
    g = np.random.default_rng(0)
    D = 16
    x = g.standard_normal((400, D))
    m, c = R.mean_cov(*R.stats(x))
    assert np.allclose(c, np.cov(x, rowvar=False), rtol=1e-10, atol=1e-12)
    assert abs(R.fid_from_moments(m, c, m, c)) <= 1e-9 * np.trace(c)                    # equal statistics -> 0
    delta = g.standard_normal(D)
    want = float(delta @ delta)
    assert abs(R.fid_from_moments(m + delta, c, m, c) - want) <= 1e-9 * (want + np.trace(c))   # mean shift only
    eye = np.eye(D)
    for s in (0.25, 1.0, 3.0):
        assert abs(R.fid_from_moments(m, eye, m, s * s * eye) - D * (1 - s) ** 2) <= 1e-10 * D * (1 + s * s)
    assert abs(R.fid(x, x + delta) - want) <= 1e-8 * (want + np.trace(c))


def test_fid_eigvals_form_equals_sqrtm_form():
    g = np.random.default_rng(1)
    D, N = 64, 3000
    a = g.standard_normal((N, D)) @ g.standard_normal((D, D))
    b = g.standard_normal((N, D)) @ g.standard_normal((D, D)) * 0.8 + 0.3
    ma, ca = R.mean_cov(*R.stats(a))
    mb, cb = R.mean_cov(*R.stats(b))
    f1, f2 = R.fid_from_moments(ma, ca, mb, cb), R.fid_sqrtm(ma, ca, mb, cb)
    assert f1 > 0 and abs(f1 - f2) <= 1e-9 * abs(f2)


def test_precision_recall_restatement_closed_forms_and_sklearn():
    from sklearn.neighbors import NearestNeighbors
    g = np.random.default_rng(2)
    x = g.standard_normal((300, 8))
    r = R.precision_recall(x, x.copy(), 3)
    assert r["precision"] == 1.0 and r["recall"] == 1.0 and r["f1"] == 1.0              # identical sets
    far = g.standard_normal((200, 8)) + 100.0
    r = R.precision_recall(x, far, 3)
    assert r["precision"] == 0.0 and r["recall"] == 0.0 and r["f1"] == 0.0              # two far-apart clusters
    for k in (1, 3, 8):
        dist, _ = NearestNeighbors(n_neighbors=k + 1, algorithm="brute").fit(x).kneighbors(x)   # column 0: the row itself
        assert np.allclose(R.knn_radius2(x, k), dist[:, k] ** 2, rtol=1e-10, atol=1e-14)
    dup = np.concatenate([x[:5], x])                                                    # duplicated rows: radius 0 at k = 1
    assert (R.knn_radius2(dup, 1)[:5] == 0).all() and (R.knn_radius2(dup, 1)[10:] > 0).all()


# ---- 3: frechet_distance on host-made statistics --------------------------------------------------------------------
def _host_stats(M, x):
    s, o, n = R.stats(x)
    fs = M.FeatureStats(x.shape[1], device="cpu")
    return fs.load_state_dict({"sum": torch.from_numpy(s), "outer": torch.from_numpy(o), "n": torch.tensor(n)})


def test_frechet_distance_on_host_made_state_equals_the_restatement():
    M = import_module(PKG + ".metrics")
    g = np.random.default_rng(3)
    D = 37
    real = (g.standard_normal((500, D)) @ g.standard_normal((D, D))).astype(np.float32)
    fake = (g.standard_normal((300, D)) @ g.standard_normal((D, D)) * 0.7 + 0.2).astype(np.float32)
    a, b = _host_stats(M, real), _host_stats(M, fake)
    want = R.fid(real, fake)
    got = M.frechet_distance(a, b)
    assert want > 0 and abs(got - want) <= 1e-10 * want
    m, c = R.mean_cov(*R.stats(real))
    assert np.array_equal(a.mean(), m) and np.allclose(a.cov(), c, rtol=1e-12, atol=0)
    # merge: the statistics are additive
    both = _host_stats(M, real[:200]).merge(_host_stats(M, real[200:]))
    assert both.n == 500 and np.allclose(both.cov(), c, rtol=1e-9, atol=1e-12)
    # state_dict round trip
    again = M.FeatureStats(D, device="cpu").load_state_dict(a.state_dict())
    assert again.n == a.n and torch.equal(again.outer, a.outer) and again.outer is not a.outer
    with pytest.raises(RuntimeError):
        M.frechet_distance(a, _host_stats(M, real[:, :5]))
    with pytest.raises(RuntimeError):
        M.FeatureStats(D, device="cpu").cov()


# ---- 4: surface ----------------------------------------------------------------------------------------------------
def test_package_surface_and_no_cpu_path():
    import vaegan_amd as V
    for name in ("metrics", "FeatureStats", "frechet_distance", "precision_recall", "encoder_features"):
        assert hasattr(V, name) and name in V.__all__, name
    assert V.FeatureStats is V.metrics.FeatureStats
    ops = import_module(PKG + ".ops")
    x = torch.zeros(10, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.feat_stats_accum(x, torch.zeros(4, dtype=torch.float64), torch.zeros(4, 4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.knn_radius2(x, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.manifold_cover(x, x, torch.zeros(10))
    with pytest.raises(RuntimeError, match="no CPU path"):
        V.precision_recall(x, x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        V.FeatureStats(4, device="cpu").update(x)
    e = V.Encoder([3, 64, 64], 100)
    with pytest.raises(RuntimeError, match="no CPU path"):
        V.encoder_features(e)(torch.zeros(2, 3, 64, 64, dtype=torch.uint8))
    with pytest.raises(RuntimeError):
        V.encoder_features(e, part="sigma")
    import inspect
    sig = inspect.signature(V.evaluate_generation).parameters
    assert sig["feature_fn"].default is None and sig["k"].default == 3 and sig["real_stats"].default is None
    assert inspect.signature(V.validation_epoch).parameters["feature_fn"].default is None
