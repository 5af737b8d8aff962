"""CPU: the Kernel Inception Distance without a GPU.  (1) the f64 numpy restatement tests/_kid_ref.py -- the yardstick of
the GPU tests -- against a closed form, against sklearn's polynomial_kernel, under a permutation of a subset and on a
statistical sanity case; (2) the C ABI: the two new symbols, the header's workspace formula, host-side argument
validation before any launch; (3) metrics.kid_subsets / metrics.kernel_distance: the host draw and the loud failures.
Parity with the torchmetrics package itself is unpinned: it is not installed."""
import ctypes
import inspect
import os
import re
from importlib import import_module

import numpy as np
import pytest
import torch

import _kid_ref as K

PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1: the restatement against independent forms -----------------------------------------------------------------------
def test_degree_1_coef_0_closed_form():
    """k = gamma a.c: sum_{i != j} x_i.x_j = |sum x|^2 - sum |x_i|^2 and sum_{ij} x_i.y_j = (sum x).(sum y)."""
    g = np.random.default_rng(0)
    m, D, gamma = 61, 23, 0.37
    x, y = g.standard_normal((m, D)), g.standard_normal((m, D)) + 0.5
    s0, s1, s2 = K.poly_mmd_sums(x, y, 1, gamma, 0.0)
    sx, sy = x.sum(0), y.sum(0)
    w0, w1, w2 = gamma * (sx @ sx - (x * x).sum()), gamma * (sy @ sy - (y * y).sum()), gamma * (sx @ sy)
    scale = gamma * (np.abs(x).sum(0) @ np.abs(x).sum(0) + np.abs(y).sum(0) @ np.abs(y).sum(0))
    assert abs(s0 - w0) <= 1e-13 * scale and abs(s1 - w1) <= 1e-13 * scale and abs(s2 - w2) <= 1e-13 * scale
    want = (w0 + w1) / (m * (m - 1)) - 2 * w2 / m ** 2
    assert abs(K.score_from_sums(s0, s1, s2, m) - want) <= 1e-13 * scale / m ** 2


def test_kernel_equals_sklearn_polynomial_kernel():
    pk = pytest.importorskip("sklearn.metrics.pairwise").polynomial_kernel
    g = np.random.default_rng(1)
    x, y = g.standard_normal((40, 17)), g.standard_normal((33, 17))
    for degree, gamma, coef in ((3, 1.0 / 17, 1.0), (2, 0.5, 0.0), (4, 0.1, 2.0), (1, 1.0, -1.0)):
        assert np.allclose(K.poly_kernel(x, y, degree, gamma, coef), pk(x, y, degree=degree, gamma=gamma, coef0=coef),
                           rtol=1e-12, atol=1e-14)


def test_score_is_invariant_under_a_permutation_of_a_subset():
    g = np.random.default_rng(2)
    real, fake = K.gauss_feats(120, 19, 3), K.gauss_feats(90, 19, 4)
    ir, jf = K.tables(120, 2, 50, 5), K.tables(90, 2, 50, 6)
    sc, _, _, sums = K.kid(real, fake, ir, jf, 3, None, 1.0)
    ir2, jf2 = ir.copy(), jf.copy()
    ir2[0], jf2[1] = ir[0][g.permutation(50)], jf[1][g.permutation(50)]
    sc2, _, _, sums2 = K.kid(real, fake, ir2, jf2, 3, None, 1.0)
    ds, dsc = K.kid_bounds(real, fake, ir, jf, 3, 1.0 / 19, 1.0)
    assert (np.abs(sums - sums2) <= ds).all() and (np.abs(sc - sc2) <= dsc).all()


def test_statistical_sanity_on_gaussian_features():
    """m = 97, D = 200, 20 subsets: the same distribution scores 0 within 3 standard errors, a shifted and shrunk fake
    set (0.25 + 0.9 N(0, I)) scores more than 10 times the same-distribution |mean|.  The 20 subsets are DISJOINT rows of
    an N = 20 * 97 pool, so the scores are independent draws of the unbiased estimator and std / sqrt(20) is their mean's
    standard error (overlapping subsets of a small pool share the pool's own deviation and are not)."""
    g = np.random.default_rng(0)
    m, D, S = 97, 200, 20
    N = S * m
    real = g.standard_normal((N, D)).astype(np.float32)
    same = g.standard_normal((N, D)).astype(np.float32)
    shifted = (0.25 + 0.9 * g.standard_normal((N, D))).astype(np.float32)
    ir, jf = g.permutation(N).reshape(S, m).astype(np.int32), g.permutation(N).reshape(S, m).astype(np.int32)
    _, mean0, std0, _ = K.kid(real, same, ir, jf)
    _, mean1, std1, _ = K.kid(real, shifted, ir, jf)
    print("same", mean0, "+-", std0, "shifted", mean1, "+-", std1)
    assert abs(mean0) <= 3.0 * std0 / np.sqrt(S)
    assert mean1 > 10.0 * abs(mean0)


def test_mean_and_population_std():
    sc = np.array([0.5, -0.25, 1.0, 0.125])
    mean, std = K.mean_std(sc)
    assert mean == sc.mean() and abs(std - sc.std(ddof=0)) <= 1e-16
    assert K.mean_std(np.array([0.3])) == (0.3, 0.0)


# ---- 2: C ABI -------------------------------------------------------------------------------------------------------
def _lib():
    return import_module(PKG + "._lib")


def test_abi_declares_binds_and_exports_the_kid_entry_points():
    L = _lib()
    src = open(os.path.join(ROOT, "include", "vaegan_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = L.load()
    for name in ("vg_kid_scores_ws_bytes", "vg_kid_scores"):
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert int(re.search(r"#define\s+VG_ABI_VERSION\s+(\d+)", src).group(1)) == L.ABI_VERSION >= 15
    assert lib.vg_abi_version() == L.ABI_VERSION


def test_workspace_equals_the_headers_formula():
    """8 * S * (2 P + T * T), T = ceil(m / 64), P = T (T + 1) / 2: one f64 per tile, never the Gram matrix."""
    lib = _lib().load()
    for m in (2, 63, 64, 65, 97, 200, 1000, 4097, 32768):
        for S in (1, 5, 100, 4096):
            T = (m + 63) // 64
            W = T * (T + 1) + T * T
            want = 8 * S * W if S * W <= 2 ** 31 - 1 else -1
            assert lib.vg_kid_scores_ws_bytes(m, S) == want, (m, S)
    assert lib.vg_kid_scores_ws_bytes(32768, 4096) == -1                                # more than 2^31 - 1 workgroups
    assert 0 < lib.vg_kid_scores_ws_bytes(1000, 100) < 1 << 20
    for m, S in ((1, 1), (0, 5), (-3, 5), (32769, 1), (100, 0), (100, 4097), (100, -1)):
        assert lib.vg_kid_scores_ws_bytes(m, S) == -1, (m, S)


def test_c_abi_rejects_bad_arguments_on_host():
    lib = _lib().load()
    buf = ctypes.c_void_p(4096)                       # never dereferenced: every call below is rejected before a launch
    odd = ctypes.c_void_p(4100)
    big = 1 << 40

    def call(real=buf, Nr=300, fake=buf, Nf=200, D=64, ir=buf, jf=buf, S=3, m=100, degree=3, gamma=1.0, coef=1.0, sums=buf,
             scores=buf, stat=buf, ws=buf, ws_bytes=big):
        return lib.vg_kid_scores(real, Nr, fake, Nf, D, ir, jf, S, m, degree, gamma, coef, sums, scores, stat, ws, ws_bytes, None)

    assert call(m=1) == -1 and call(m=0) == -1
    assert call(m=201) == -1 and call(m=301, Nf=400) == -1                              # m > Nf, m > Nr
    assert call(Nr=40000, Nf=40000, m=32769) == -1
    assert call(D=0) == -1 and call(D=4096) == -1 and call(D=2049) == -1
    assert call(degree=0) == -1 and call(degree=9) == -1
    assert call(S=0) == -1 and call(S=4097) == -1
    assert call(gamma=float("nan")) == -1 and call(gamma=float("inf")) == -1 and call(coef=float("-inf")) == -1
    for name in ("real", "fake", "ir", "jf", "sums", "scores", "stat", "ws"):
        assert call(**{name: None}) == -1, name
    need = lib.vg_kid_scores_ws_bytes(100, 3)
    assert need == 8 * 3 * 10 and call(ws_bytes=need - 1) == -1 and call(ws_bytes=0) == -1
    for name in ("real", "fake", "sums", "scores", "stat", "ws"):
        assert call(**{name: odd}) == -2, name
    assert call(ir=ctypes.c_void_p(4098)) == -2 and call(jf=ctypes.c_void_p(4097)) == -2
    assert call(real=ctypes.c_void_p(4104)) == -2                                       # 8-byte aligned is not enough for rows


# ---- 3: Python ------------------------------------------------------------------------------------------------------
def test_kid_subsets_is_the_documented_host_draw():
    M = import_module(PKG + ".metrics")
    Nr, Nf, S, m = 57, 41, 6, 23
    ir, jf = M.kid_subsets(Nr, Nf, S, m, seed=7)
    assert ir.dtype == np.int32 and jf.dtype == np.int32 and ir.shape == (S, m) and jf.shape == (S, m)
    again = M.kid_subsets(Nr, Nf, S, m, seed=7)
    assert np.array_equal(ir, again[0]) and np.array_equal(jf, again[1])                # reproducible per seed
    other = M.kid_subsets(Nr, Nf, S, m, seed=8)
    assert not np.array_equal(ir, other[0])
    g = np.random.Generator(np.random.PCG64(7))                                         # real before fake, subset by subset
    for s in range(S):
        assert np.array_equal(ir[s], g.permutation(Nr)[:m]) and np.array_equal(jf[s], g.permutation(Nf)[:m])
    for t, N in ((ir, Nr), (jf, Nf)):
        assert t.min() >= 0 and t.max() < N
        assert all(len(set(row.tolist())) == m for row in t)                            # a duplicate-free prefix
    full = M.kid_subsets(9, 9, 2, 9, seed=1)
    assert all(sorted(row.tolist()) == list(range(9)) for t in full for row in t)
    with pytest.raises(ValueError):
        M.kid_subsets(10, 5, 2, 6)


def test_kernel_distance_surface_and_loud_failures():
    import vaegan_amd as V
    M = V.metrics
    assert V.kernel_distance is M.kernel_distance and "kernel_distance" in V.__all__
    p = inspect.signature(M.kernel_distance).parameters
    assert [p[k].default for k in ("subsets", "subset_size", "degree", "gamma", "coef", "seed", "idx_real", "idx_fake")] == \
        [100, 1000, 3, None, 1.0, 0, None, None]
    for fn in (V.evaluate_generation, V.validation_epoch):
        q = inspect.signature(fn).parameters
        assert (q["kid_subsets"].default, q["kid_subset_size"].default, q["kid_seed"].default) == (None, 1000, 0)
    x = torch.zeros(10, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.kernel_distance(x, x, subsets=2, subset_size=4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        V.ops.kid_scores(x, x, torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32))
    with pytest.raises(RuntimeError):
        M.FeaturePass(lambda u8: None, False).kid(2, 4)
    with pytest.raises(RuntimeError, match="feature_fn"):
        V.evaluate_generation(None, [], kid_subsets=4)
    with pytest.raises(RuntimeError, match="feature_fn"):
        V.validation_epoch(None, None, [], kid_subsets=4)


class _FakeDeviceFeats(torch.Tensor):
    """A host tensor that answers is_cuda: lets the argument checks that come BEFORE any device work run here."""
    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t)

    @property
    def is_cuda(self):
        return True


def test_kernel_distance_validates_sizes_and_injected_tables_on_the_host():
    M = import_module(PKG + ".metrics")
    real, fake = _FakeDeviceFeats(torch.zeros(12, 4)), _FakeDeviceFeats(torch.zeros(9, 4))
    with pytest.raises(ValueError, match="subset_size"):
        M.kernel_distance(real, fake, subsets=2, subset_size=10)                        # > min(Nr, Nf)
    ok = np.zeros((2, 5), np.int32)
    for bad in (np.full((2, 5), 9, np.int32), np.full((2, 5), -1, np.int32)):
        with pytest.raises(ValueError, match="row indices"):
            M.kernel_distance(real, fake, idx_real=ok, idx_fake=bad)                    # out of range for fake (9 rows)
    with pytest.raises(ValueError, match="row indices"):
        M.kernel_distance(real, fake, idx_real=np.full((2, 5), 12, np.int64), idx_fake=ok)
    with pytest.raises(ValueError):
        M.kernel_distance(real, fake, idx_real=ok, idx_fake=np.zeros((2, 4), np.int32))    # shapes differ
    with pytest.raises(ValueError):
        M.kernel_distance(real, fake, idx_real=ok.astype(np.float32), idx_fake=ok)      # not integers
    with pytest.raises(ValueError):
        M.kernel_distance(real, fake, idx_real=ok, idx_fake=None)
