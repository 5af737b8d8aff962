"""CPU: the Gaussian-mixture prior before any kernel runs.  (1) tests/_gmm_ref.py's EM loop -- the loop
latent.GaussianMixturePrior.fit runs, with the shifted one-pass M-step -- against scikit-learn's GaussianMixture from the
same initialisation; (2) the exact-input tables of the GPU tests are exact in f64 (held against integer / Fraction
arithmetic), so a bitwise comparison there has no blind spot; (3) the C ABI declarations, the ctypes table, host-side
argument validation, the package exports and the "no CPU path" errors."""
import ctypes
import inspect
import os
import re
from fractions import Fraction
from importlib import import_module

import numpy as np
import pytest
import torch
from sklearn.mixture import GaussianMixture

import _gmm_ref as R

PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vg_gmm_log_resp", "vg_gmm_moments_ws_bytes", "vg_gmm_moments", "vg_gmm_sample")


# ---- 1. the restated EM loop against scikit-learn ---------------------------------------------------------------------
@pytest.mark.parametrize("N,D,K,offset", R.FIT_CASES)
def test_restated_fit_follows_scikit_learn(N, D, K, offset):
    """Measured on the development host over the five cases: at most 1.15e-12 (on precisions_cholesky_; weights, means and
    lower_bound_ below 1e-14), 7 - 11 iterations each.  Asserted: 64 x 1.15e-12 = 7.4e-11; the margin covers another host's
    BLAS summation order."""
    x = R.make_mixture(N, D, K, offset)
    idx = R.default_init(N, K)
    p0 = R.init_params(x, idx, 1e-6)
    p = R.fit(x, idx)
    g = GaussianMixture(K, covariance_type="full", weights_init=p0["weights"], means_init=p0["means"],
                                precisions_init=p0["precisions"], reg_covar=1e-6, tol=1e-3, max_iter=100)
    g.fit(x.astype(np.float64))                                          # the f32 values, computed in f64
    assert (p["n_iter"], p["converged"]) == (g.n_iter_, g.converged_)
    assert 3 <= p["n_iter"] < 100
    dev = {"weights": R.rel_dev(p["weights"], g.weights_), "means": R.rel_dev(p["means"], g.means_),
           "prec_chol": R.rel_dev(p["prec_chol"], g.precisions_cholesky_),
           "lower_bound": abs(p["lower_bound"] - g.lower_bound_) / abs(g.lower_bound_)}
    print("deviation from scikit-learn", (N, D, K, offset), dev)
    for name, v in dev.items():
        assert v <= R.FIT_BOUND, (name, v)
    assert np.array_equal(p["cdf"], np.cumsum(p["weights"])) and np.allclose(p["cdf"][-1], 1.0, atol=1e-14)
    for k in range(K):                                                   # the factors are factors
        assert np.allclose(p["cov_chol"][k] @ p["cov_chol"][k].T, p["covariances"][k], rtol=1e-10, atol=1e-12)
        assert np.array_equal(p["prec_chol"][k], np.triu(p["prec_chol"][k]))


def test_global_variance_is_the_column_variance():
    x = R.make_mixture(600, 5, 2, 100.0)
    assert np.allclose(R.global_variance(x, 17), x.astype(np.float64).var(axis=0), rtol=1e-12)


# ---- 2. the exact-input tables are exact ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,K", [(63, 5, 3), (257, 17, 1), (40, 100, 10)])
def test_exact_estep_table_is_exact_in_f64(N, D, K):
    x, mean, U, log_coef = R.exact_estep_inputs(N, D, K)
    lp, ln, resp = R.log_resp(x, mean, U, log_coef)
    d = x.astype(np.int64)[:, None, :] - mean.astype(np.int64)[None]                      # [N,K,D]
    y2 = np.einsum("nki,kij->nkj", d, (2 * U).astype(np.int64))                           # 2 y, integers
    q = (y2 * y2).sum(axis=2)                                                             # 4 sum y^2
    assert np.abs(q).max() < 2 ** 52
    for n in range(N):
        for k in range(K):
            want = Fraction(float(log_coef[k])) - Fraction(int(q[n, k]), 8)
            assert Fraction(float(lp[n, k])) == want
    if K == 1:
        assert np.array_equal(ln, lp[:, 0]) and np.all(resp == 1.0)


@pytest.mark.parametrize("N,D,K", [(63, 5, 3), (1000, 17, 3), (257, 100, 10)])
def test_exact_moment_table_is_exact_in_f64(N, D, K):
    x, shift, resp, log_norm = R.exact_moment_inputs(N, D, K)
    assert np.array_equal(resp.sum(axis=1), np.ones(N)) and np.array_equal(resp * 8, np.round(resp * 8))
    nk, s1, s2, ll = R.moments(x, shift, resp, log_norm)
    r8 = np.round(resp * 8).astype(np.int64)
    for k in range(K):
        d = x.astype(np.int64) - shift[k].astype(np.int64)
        assert nk[k] * 8 == r8[:, k].sum()
        assert np.array_equal(s1[k] * 8, (r8[:, k, None] * d).sum(axis=0))
        assert np.array_equal(s2[k] * 8, (r8[:, k, None] * d).T @ d)
    assert ll * 4 == np.round(log_norm * 4).astype(np.int64).sum()


def test_exact_sample_table_is_exact_and_hits_the_edges():
    cdf, mean, chol, u, eps = R.exact_sample_inputs(64, 17, 3)
    comp, z64, z32 = R.sample(cdf, mean, chol, u, eps)
    assert u[0] == 0.0 and comp[0] == 0
    assert u[2] == cdf[-1] == 1.0 - 2.0 ** -53 and comp[2] == 2                            # past the end: clamped
    assert u[3] == cdf[0] and comp[3] == 1                                                 # side = "right"
    assert np.array_equal(z32.astype(np.float64), z64)                                     # the f32 rounding is exact too
    L32 = np.round(chol * 4).astype(np.int64)
    e8 = np.round(eps.astype(np.float64) * 8).astype(np.int64)
    for j in range(64):
        want = np.round(mean[comp[j]] * 4).astype(np.int64) * 8 + np.tril(L32[comp[j]]) @ e8[j]     # 32 z
        assert np.array_equal(z64[j] * 32, want)


# ---- 3. the library, host side --------------------------------------------------------------------------------------
def test_header_declares_and_binding_table_binds_the_new_entry_points():
    L = import_module(PKG + "._lib")
    src = open(os.path.join(ROOT, "include", "vaegan_hip.h")).read()
    lib = L.load()
    for name in NEW:
        assert re.search(r"\b(int|int64_t)\s+" + name + r"\s*\(", src), name
        assert name in L.SIGNATURES, name
        assert hasattr(lib, name), name
    m = re.search(r"#define\s+VG_ABI_VERSION\s+(\d+)", src)
    assert int(m.group(1)) == L.ABI_VERSION >= 28 and lib.vg_abi_version() == L.ABI_VERSION
    ids = {n: int(re.search(r"#define\s+" + n + r"\s+(\d+)", src).group(1)) for n in ("VG_DRAW_GMM_U", "VG_DRAW_GMM_EPS")}
    assert ids == {"VG_DRAW_GMM_U": 40, "VG_DRAW_GMM_EPS": 41}
    ops = import_module(PKG + ".ops")
    assert (ops.DRAW_GMM_U, ops.DRAW_GMM_EPS) == (40, 41)
    for text in ("Gaussian-mixture prior", "CLAMPED to K - 1", "precisions_cholesky_"):
        assert text in src


def test_c_abi_of_the_gmm_entry_points_rejects_bad_arguments_on_host():
    L = import_module(PKG + "._lib")
    lib = L.load()
    b = ctypes.c_void_p(256)                                             # never dereferenced: validation comes first
    odd = ctypes.c_void_p(260)
    big = 1 << 40
    # vg_gmm_moments_ws_bytes
    assert lib.vg_gmm_moments_ws_bytes(200000, 100, 10) > 0
    for bad in ((0, 8, 3), (1 << 31, 8, 3), (10, 0, 3), (10, 257, 3), (10, 8, 0), (10, 8, 65)):
        assert lib.vg_gmm_moments_ws_bytes(*bad) == -1, bad
    assert lib.vg_gmm_moments_ws_bytes(2 ** 31 - 1, 256, 64) > 0
    # vg_gmm_log_resp(x, N, D, stride, K, mean, prec_chol, log_coef, log_prob, log_norm, resp, stream)
    def e(x=b, N=10, D=8, stride=8, K=3, mean=b, U=b, coef=b, lp=b, ln=b, rs=b):
        return lib.vg_gmm_log_resp(x, N, D, stride, K, mean, U, coef, lp, ln, rs, None)
    for kw in (dict(x=None), dict(mean=None), dict(U=None), dict(coef=None), dict(N=0), dict(N=1 << 31), dict(D=0),
               dict(D=257, stride=257), dict(K=0), dict(K=65), dict(stride=7), dict(lp=None, ln=None, rs=None)):
        assert e(**kw) == -1, kw
    assert e(mean=odd) == -2 and e(rs=odd) == -2
    # vg_gmm_moments(x, N, D, stride, K, shift, resp, log_norm, nk, s1, s2, loglik, ws, ws_bytes, stream)
    def m(x=b, N=10, D=8, stride=8, K=3, shift=b, resp=b, ln=b, nk=b, s1=b, s2=b, ll=b, ws=b, wsb=big):
        return lib.vg_gmm_moments(x, N, D, stride, K, shift, resp, ln, nk, s1, s2, ll, ws, wsb, None)
    for kw in (dict(x=None), dict(shift=None), dict(resp=None), dict(nk=None), dict(s1=None), dict(s2=None), dict(ws=None),
               dict(N=0), dict(N=1 << 31), dict(D=0), dict(D=257, stride=257), dict(K=0), dict(K=65), dict(stride=7),
               dict(ln=None), dict(wsb=8), dict(wsb=lib.vg_gmm_moments_ws_bytes(10, 8, 3) - 1)):
        assert m(**kw) == -1, kw                                          # ln=None with loglik asked for: refused
    assert m(s2=odd) == -2 and m(ws=odd) == -2
    # vg_gmm_sample(cdf, mean, cov_chol, K, D, n, u, eps, rng, comp, z32, z, ZP, dtype, stream)
    def s(cdf=b, mean=b, chol=b, K=3, D=8, n=4, u=b, eps=b, rng=None, comp=b, z32=b, z=None, ZP=0, dt=0):
        return lib.vg_gmm_sample(cdf, mean, chol, K, D, n, u, eps, rng, comp, z32, z, ZP, dt, None)
    for kw in (dict(cdf=None), dict(mean=None), dict(chol=None), dict(K=0), dict(K=65), dict(D=0), dict(D=257), dict(n=0),
               dict(comp=None, z32=None), dict(u=None), dict(eps=None), dict(z=b, ZP=4)):
        assert s(**kw) == -1, kw                                          # u / eps missing without a generator; ZP < D
    assert s(z=b, ZP=8, dt=7) == -3
    assert s(z=odd, ZP=8, dt=1) == -2 and s(cdf=odd) == -2


def test_package_exports_and_host_tensors_are_refused():
    import vaegan_amd as V
    assert "GaussianMixturePrior" in V.__all__ and V.GaussianMixturePrior is V.latent.GaussianMixturePrior
    assert "GaussianMixturePrior" in V.__doc__
    ops = import_module(PKG + ".ops")
    x = torch.randn(32, 4)
    f64 = dict(dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.gmm_log_resp(x, torch.zeros(2, 4, **f64), torch.zeros(2, 4, 4, **f64), torch.zeros(2, **f64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.gmm_moments(x, torch.zeros(2, 4, **f64), torch.zeros(32, 2, **f64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.gmm_sample(torch.ones(2, **f64), torch.zeros(2, 4, **f64), torch.zeros(2, 4, 4, **f64), 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        V.GaussianMixturePrior.fit(x, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        V.GaussianMixturePrior(torch.ones(1, **f64), torch.zeros(1, 4, **f64), *(torch.zeros(1, 4, 4, **f64),) * 3,
                               torch.ones(1, **f64))


def test_fit_validates_its_arguments_before_any_launch():
    import vaegan_amd as V

    class OnDevice:                                                      # fit looks at the description before any launch
        is_cuda, dtype, shape = True, torch.float32, (5, 4)

        def dim(self):
            return 2

    x = OnDevice()
    with pytest.raises(RuntimeError, match="cannot initialise"):
        V.GaussianMixturePrior.fit(x, n_components=6)
    for bad in ([0, 0, 1], [0, 1], [0, 1, 5], [-1, 0, 1], [0.0, 1.0, 2.0]):
        with pytest.raises(RuntimeError, match="init_idx"):
            V.GaussianMixturePrior.fit(x, n_components=3, init_idx=bad)
    with pytest.raises(RuntimeError, match="n_components"):
        V.GaussianMixturePrior.fit(x, n_components=0)


def test_existing_defaults_of_evaluate_generation_did_not_move():
    import vaegan_amd as V
    sig = inspect.signature(V.evaluate_generation)
    assert list(sig.parameters) == ["decoder", "val_loader", "prior", "noise_fn", "feature_fn", "k", "real_stats",
                                    "kid_subsets", "kid_subset_size", "kid_seed"]
    got = {n: p.default for n, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert got == {"prior": None, "noise_fn": None, "feature_fn": None, "k": 3, "real_stats": None, "kid_subsets": None,
                   "kid_subset_size": 1000, "kid_seed": 0}
    sig = inspect.signature(V.sample_images)
    assert [(n, p.default) for n, p in sig.parameters.items()][1:] == [("z", None), ("n", 64), ("prior", None),
                                                                        ("grid_cols", 0)]
