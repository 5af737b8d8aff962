"""GPU: the Gaussian-mixture prior (vg_gmm_log_resp, vg_gmm_moments, vg_gmm_sample and latent.GaussianMixturePrior above
them) against the numpy f64 restatement tests/_gmm_ref.py.  Exact-input tables (tests/test_gmm_cpu.py shows that every
intermediate of theirs is exact in f64) are compared bit for bit; random inputs within bounds counted from the roundings.
No expectation is taken from the kernel under test.  The kernel-level tests call the C entry points themselves
(raw_log_resp, raw_moments, raw_sample below) over outputs and workspace PRE-FILLED WITH NaN (comp, an int32, with -7), so
a stale right answer in recycled memory cannot pass; the ops wrappers are held against those calls bit for bit.

exp / log: the ROCm installation carries no accuracy table for the device's f64 exp and log, so 2 ulp each is ASSUMED
(ULP_EXP, ULP_LOG); numpy's own are taken as 1 ulp."""
import io
import math

import numpy as np
import pytest
import torch

import _gmm_ref as R
import vaegan_amd as V
from test_gpu_data import jpeg_folder  # noqa: F401  (fixture: 45 generated 64 x 64 JPEGs)
from test_gpu_parity import build

pytestmark = pytest.mark.gpu
DEV = "cuda"
ops, data, G = V.ops, V.data, V.geometry
U = 2.0 ** -52                                        # one ulp, relative
ULP_EXP = ULP_LOG = 2                                 # assumed for the device (see the module docstring)


def dev64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV)


def dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def strided(x, pad=7):
    """The same rows as columns [0, D) of a wider device matrix whose other columns are NaN."""
    N, D = x.shape
    wide = torch.full((N, D + pad), float("nan"), dtype=torch.float32, device=DEV)
    wide[:, :D] = dev32(x)
    return wide[:, :D]


def bits(t):
    a = t.cpu().numpy()
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def same_bits(got, want):
    want = np.ascontiguousarray(want)
    return np.array_equal(bits(got), want.view(np.int64 if want.dtype == np.float64 else np.int32))


def nan64(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)


def rows_of(x):
    N, D = x.shape
    return N, D, (x.stride(0) if N > 1 else D)


def raw_log_resp(x, mean, Uc, coef):
    """vg_gmm_log_resp over NaN-filled outputs -> (log_prob, log_norm, resp)."""
    L = ops.L
    N, D, stride = rows_of(x)
    K = mean.shape[0]
    lp, ln, rs = nan64(N, K), nan64(N), nan64(N, K)
    L.check(L.load().vg_gmm_log_resp(x.data_ptr(), N, D, stride, K, mean.data_ptr(), Uc.data_ptr(), coef.data_ptr(),
                                     lp.data_ptr(), ln.data_ptr(), rs.data_ptr(), L.stream_ptr()), "vg_gmm_log_resp")
    return lp, ln, rs


def raw_moments(x, shift, resp, ln=None):
    """vg_gmm_moments over NaN-filled outputs and a NaN-filled workspace -> (nk, s1, s2, loglik or None)."""
    L = ops.L
    lib = L.load()
    N, D, stride = rows_of(x)
    K = shift.shape[0]
    nk, s1, s2, ll = nan64(K), nan64(K, D), nan64(K, D, D), (nan64(1) if ln is not None else None)
    nbytes = lib.vg_gmm_moments_ws_bytes(N, D, K)
    ws = nan64(nbytes // 8)
    L.check(lib.vg_gmm_moments(x.data_ptr(), N, D, stride, K, shift.data_ptr(), resp.data_ptr(), L.ptr(ln), nk.data_ptr(),
                               s1.data_ptr(), s2.data_ptr(), L.ptr(ll), ws.data_ptr(), nbytes, L.stream_ptr()),
            "vg_gmm_moments")
    return nk, s1, s2, ll


def raw_sample(cdf, mean, chol, n, u, eps, state, ZP, dtype):
    """vg_gmm_sample over pre-filled outputs (comp -7, z32 and z NaN) -> (comp, z32, z [n, ZP])."""
    L = ops.L
    K, D = mean.shape
    comp = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    z32 = torch.full((n, D), float("nan"), dtype=torch.float32, device=DEV)
    z = torch.full((n, ZP), float("nan"), dtype=ops.TORCH_DT[dtype], device=DEV)
    L.check(L.load().vg_gmm_sample(cdf.data_ptr(), mean.data_ptr(), chol.data_ptr(), K, D, n, L.ptr(u), L.ptr(eps),
                                   L.ptr(state), comp.data_ptr(), z32.data_ptr(), z.data_ptr(), ZP, dtype, L.stream_ptr()),
            "vg_gmm_sample")
    return comp, z32, z


# (N, D, K, strided view): ragged rows, D below / at / above a tile and the widest, K = 1, more than one workgroup, the
# 32-row tiling (D = 256 or D = 100 with K = 64: the 64-row tile's LDS does not fit)
SHAPES = [(1, 1, 1, False), (63, 5, 3, False), (63, 5, 3, True), (257, 17, 1, False), (1000, 16, 3, False),
          (257, 100, 10, False), (70, 256, 2, False), (70, 100, 64, False)]


# ---- 1: the quadratic form, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,K,view", SHAPES)
def test_log_prob_is_exact_on_exact_inputs(N, D, K, view):
    x, mean, Uc, coef = R.exact_estep_inputs(N, D, K)
    want_lp, want_ln, want_resp = R.log_resp(x, mean, Uc, coef)
    xd = strided(x) if view else dev32(x)
    args = (xd, dev64(mean), dev64(Uc), dev64(coef))
    lp, ln, resp = raw_log_resp(*args)
    assert same_bits(lp, want_lp)
    assert not torch.isnan(ln).any() and not torch.isnan(resp).any()                       # every element written
    if K == 1:
        assert same_bits(ln, want_lp[:, 0]) and same_bits(resp, np.ones((N, 1)))
    for got, raw in zip(ops.gmm_log_resp(*args, want_log_prob=True), (lp, ln, resp)):      # the wrapper: the same bits
        assert got.shape == raw.shape and torch.equal(got, raw)
    # entries below the diagonal are never read
    junk = Uc + np.tril(np.full((D, D), np.nan), -1)
    lp2, ln2, resp2 = raw_log_resp(xd, dev64(mean), dev64(junk), dev64(coef))
    assert same_bits(lp2, want_lp) and torch.equal(ln2, ln) and torch.equal(resp2, resp)


# ---- 2: log_norm and resp on random inputs ------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,K", [(63, 5, 3), (257, 17, 10), (1000, 100, 10), (70, 256, 2)])
def test_log_norm_and_resp_within_the_counted_bound(N, D, K):
    """log_prob against the restatement: two f64 evaluations of y = d U (at most D + 1 roundings per entry each) and of
    sum y^2.  log_norm and resp against the restatement fed the DEVICE's log_prob, so only the K exponentials, the K - 1
    additions, the logarithm and the final addition differ.  With U = 2^-52, one ulp: an exponential is off by at most
    ULP_EXP U on the device and U in numpy, (ULP_EXP + 1) U between them; each of the K - 1 additions rounds by U / 2 on
    either side, (K - 1) U between them; the logarithm (of a sum in [1, K]) by (ULP_LOG + 1) U log K; the final addition by
    U / 2 |log_norm| on either side.  All on NaN-filled outputs."""
    x = R.make_mixture(N, D, min(K, 4))
    p = R.init_params(x, R.default_init(N, K), 1e-6)
    r = np.random.default_rng(N + D + K)
    Uc = p["prec_chol"] + np.triu(r.normal(size=(K, D, D)) * 0.1 / math.sqrt(D), 1)
    mean, coef = p["means"], p["log_coef"]
    lp, ln, resp = raw_log_resp(dev32(x), dev64(mean), dev64(Uc), dev64(coef))
    lp, ln, resp = lp.cpu().numpy(), ln.cpu().numpy(), resp.cpu().numpy()
    want_lp, _, _ = R.log_resp(x, mean, Uc, coef)
    A = np.stack([np.abs(x.astype(np.float64) - mean[k]) @ np.abs(Uc[k]) for k in range(K)], axis=1)      # [N,K,D]
    bound_lp = 0.5 * 5 * (D + 2) * U * (A * A).sum(axis=2) + U * np.abs(want_lp)
    print("log_prob: worst error / bound", float((np.abs(lp - want_lp) / bound_lp).max()))
    assert np.all(np.abs(lp - want_lp) <= bound_lp)
    # the log-sum-exp of the device's own log_prob
    m = lp.max(axis=1)
    s = np.zeros(N)
    for k in range(K):
        s = s + np.exp(lp[:, k] - m)
    want_ln = m + np.log(s)
    bound_ln = U * ((ULP_EXP + 1) + (K - 1) + (ULP_LOG + 1) * max(math.log(K), U) + np.abs(want_ln))
    print("log_norm: worst error / bound", float((np.abs(ln - want_ln) / bound_ln).max()))
    assert np.all(np.abs(ln - want_ln) <= bound_ln)
    arg = lp - want_ln[:, None]
    want_resp = np.exp(arg)
    bound_resp = want_resp * (bound_ln[:, None] + U * np.abs(arg) + (ULP_EXP + 1) * U) + 2.0 ** -1074
    print("resp: worst error / bound", float((np.abs(resp - want_resp) / bound_resp).max()))
    assert np.all(np.abs(resp - want_resp) <= bound_resp)
    assert np.all(np.abs(resp.sum(axis=1) - 1.0) <= (K + 4) * U + K * bound_ln)


def test_a_nan_row_gives_a_nan_log_norm_and_leaves_the_others_alone():
    x, mean, Uc, coef = R.exact_estep_inputs(63, 5, 3)
    want = R.log_resp(x, mean, Uc, coef)[1]
    x[17, 2] = np.nan
    _, ln, _ = raw_log_resp(dev32(x), dev64(mean), dev64(Uc), dev64(coef))
    ln = ln.cpu().numpy()
    assert np.isnan(ln[17]) and np.isfinite(np.delete(ln, 17)).all()
    got = R.log_resp(np.delete(x, 17, axis=0), mean, Uc, coef)[1]
    assert np.allclose(np.delete(ln, 17), got, rtol=0, atol=64 * U * np.abs(want).max())


# ---- 3: the moments -------------------------------------------------------------------------------------------------
MOMENT_SHAPES = [(1, 1, 1, False), (63, 5, 3, False), (63, 5, 3, True), (1000, 17, 3, False), (257, 100, 10, False),
                 (300, 256, 2, False), (257, 16, 1, False)]


@pytest.mark.parametrize("N,D,K,view", MOMENT_SHAPES)
def test_moments_are_exact_on_exact_inputs(N, D, K, view):
    x, shift, resp, ln = R.exact_moment_inputs(N, D, K)
    want = R.moments(x, shift, resp, ln)
    xd = strided(x) if view else dev32(x)
    args = (xd, dev64(shift), dev64(resp), dev64(ln))
    nk, s1, s2, ll = raw_moments(*args)
    assert same_bits(nk, want[0]) and same_bits(s1, want[1]) and same_bits(s2, want[2])
    assert same_bits(ll, np.array([want[3]]))
    nk, s1, s2, ll = raw_moments(*args[:3])                                                # without the log-likelihood
    assert ll is None and same_bits(nk, want[0]) and same_bits(s1, want[1]) and same_bits(s2, want[2])
    got = ops.gmm_moments(*args)                                                           # the wrapper: the same bits
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and same_bits(got[2], want[2])
    assert same_bits(got[3], np.array([want[3]])) and ops.gmm_moments(*args[:3])[3] is None


def test_moments_split_the_rows():
    """N = 1000 is split over row parts: the workspace grows with N (the exact case (1000, 17, 3) above runs that split)."""
    lib = ops.L.load()
    assert lib.vg_gmm_moments_ws_bytes(1000, 17, 3) > lib.vg_gmm_moments_ws_bytes(63, 17, 3) > 0


@pytest.mark.parametrize("N,D,K", [(1000, 17, 3), (257, 100, 10)])
def test_moments_on_random_inputs_within_the_bound_and_repeatable(N, D, K):
    """Per entry within N 2^-53 sum |terms| of the restatement, on NaN-filled outputs; the worst error / bound is printed."""
    x = R.make_mixture(N, D, min(K, 4))
    p = R.init_params(x, R.default_init(N, K), 1e-6)
    _, ln, resp = R.log_resp(x, p["means"], p["prec_chol"], p["log_coef"])
    want = R.moments(x, p["means"], resp, ln)
    a1, a2 = R.moments_abs(x, p["means"], resp)
    args = (dev32(x), dev64(p["means"]), dev64(resp), dev64(ln))
    got = raw_moments(*args)
    e = N * 2.0 ** -53
    bounds = (e * resp.sum(axis=0), e * a1, e * a2, e * np.abs(ln).sum())
    for name, g, w, b in zip(("nk", "s1", "s2", "loglik_sum"), got, want, bounds):
        err = np.abs(g.cpu().numpy().reshape(np.shape(b)) - w)
        print(name, "worst error / bound", float(np.max(err / b)))
        assert np.all(err <= b), name
    s2 = got[2].cpu().numpy()
    assert np.array_equal(s2, s2.transpose(0, 2, 1))                                       # mirrored, not recomputed
    for again in (raw_moments(*args), ops.gmm_moments(*args)):
        for g, h in zip(got, again):
            assert np.array_equal(bits(g), bits(h))


# ---- 4: the fit -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted():
    """(x, device x, reference fit, device fit) at (3000, 100, 4); shared, never modified."""
    N, D, K = 3000, 100, 4
    x = R.make_mixture(N, D, K)
    idx = R.default_init(N, K)
    xd = dev32(x)
    return x, xd, R.fit(x, idx), V.GaussianMixturePrior.fit(xd, K, init_idx=idx)


def check_fit(ref, prior, N, D, K):
    assert (prior.n_iter, prior.converged) == (ref["n_iter"], ref["converged"])
    assert (prior.n_components, prior.latent_dim, prior.n_fitted) == (K, D, N)
    dev = {k: R.rel_dev(getattr(prior, k).cpu().numpy(), ref[k])
           for k in ("weights", "means", "covariances", "prec_chol", "cov_chol", "cdf")}
    dev["lower_bound"] = abs(prior.lower_bound - ref["lower_bound"]) / abs(ref["lower_bound"])
    print("device fit against the restatement", (N, D, K), dev)
    for name, v in dev.items():
        assert v <= R.FIT_BOUND, (name, v)
    for t in (prior.weights, prior.means, prior.covariances, prior.prec_chol, prior.cov_chol, prior.cdf):
        assert t.is_cuda and t.dtype == torch.float64


def test_fit_follows_the_restated_loop_small():
    N, D, K = 2000, 8, 3
    x = R.make_mixture(N, D, K)
    idx = R.default_init(N, K)
    check_fit(R.fit(x, idx), V.GaussianMixturePrior.fit(strided(x), K, init_idx=idx), N, D, K)
    # the default initialisation is default_rng(seed).choice
    again = V.GaussianMixturePrior.fit(dev32(x), K, seed=0)
    check_fit(R.fit(x, idx), again, N, D, K)


def test_fit_follows_the_restated_loop_at_the_latent_size(fitted):
    x, xd, ref, prior = fitted
    check_fit(ref, prior, 3000, 100, 4)
    want = R.log_resp(x, ref["means"], ref["prec_chol"], ref["log_coef"])[1]
    got = prior.score_samples(xd)
    assert got.dtype == torch.float64 and got.shape == (3000,)
    assert np.abs(got.cpu().numpy() - want).max() <= R.FIT_BOUND * np.abs(want).max()
    fresh = V.GaussianMixturePrior.from_state_dict(prior.state_dict())                      # log_coef rebuilt on the host
    assert np.abs(fresh.score_samples(xd).cpu().numpy() - want).max() <= R.FIT_BOUND * np.abs(want).max()
    assert abs(prior.score(xd) - want.mean()) <= R.FIT_BOUND * abs(want.mean())
    assert same_bits(got, prior.score_samples(xd).cpu().numpy())


def test_fit_refuses_what_em_cannot_use():
    x = R.make_mixture(600, 5, 2)
    bad = x.copy()
    bad[300, 1] = np.nan
    with pytest.raises(RuntimeError, match="reg_covar"):
        V.GaussianMixturePrior.fit(dev32(bad), 2)
    flat = x.copy()
    flat[:, 3] = 1.5
    with pytest.raises(RuntimeError, match="reg_covar"):
        V.GaussianMixturePrior.fit(dev32(flat), 2, reg_covar=0.0)
    ok = V.GaussianMixturePrior.fit(dev32(flat), 2)                                        # the default reg_covar carries it
    assert math.isfinite(ok.lower_bound) and ok.n_iter >= 1
    with pytest.raises(RuntimeError, match="cannot initialise"):
        V.GaussianMixturePrior.fit(dev32(x[:3]), 4)


# ---- 5: the sampler -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D,K,dtype", [(64, 17, 3, G.F32), (64, 17, 3, G.BF16), (9, 1, 1, G.F32), (300, 100, 10, G.BF16),
                                         (33, 256, 2, G.F32)])
def test_sampler_is_exact_on_exact_inputs(n, D, K, dtype):
    cdf, mean, chol, u, eps = R.exact_sample_inputs(n, D, K)
    comp_w, z64_w, z32_w = R.sample(cdf, mean, chol, u, eps)
    ZP = G.padc(D, dtype)
    junk = chol + np.triu(np.full((D, D), np.nan), 1)                                      # above the diagonal: never read
    args = (dev64(cdf), dev64(mean), dev64(junk), n, dev64(u), dev32(eps), None)
    comp, z32, z = raw_sample(*args, ZP, dtype)                                            # comp -7, z32 and z NaN before
    assert np.array_equal(comp.cpu().numpy(), comp_w)
    assert same_bits(z32, z32_w)
    want_z = torch.zeros(n, ZP, dtype=torch.float32)                                       # pad columns zero
    want_z[:, :D] = torch.from_numpy(z32_w)
    assert torch.equal(z.cpu(), want_z.to(ops.TORCH_DT[dtype]))
    wc, w32, wz = ops.gmm_sample(*args, want_comp=True, z=(ZP, dtype))                     # the wrapper: the same bits
    assert wc.dtype == torch.int32 and wz.shape == (n, 1, 1, ZP) and wz.dtype == ops.TORCH_DT[dtype]
    assert torch.equal(wc, comp) and torch.equal(w32, z32) and torch.equal(wz.view(n, ZP), z)
    if K >= 3 and n >= 8:
        assert comp_w[0] == 0 and comp_w[2] == K - 1 and comp_w[3] == 1                    # u = 0, the clamp, u == cdf[0]


def test_sampler_on_random_inputs_within_the_counted_bound(fitted):
    """z64: a chain of at most D fused multiply-adds and one addition on the device, a dot product and one addition in
    numpy: (D + 2) 2^-53 (|mean| + sum |L| |eps|) each; then ONE rounding to f32, 2^-24 |z|."""
    _, _, ref, prior = fitted
    n, D = 257, 100
    r = np.random.default_rng(5)
    u, eps = r.random(n), r.standard_normal((n, D)).astype(np.float32)
    cdf, mean, chol = (getattr(prior, k).cpu().numpy() for k in ("cdf", "means", "cov_chol"))
    comp_w, z64_w, _ = R.sample(cdf, mean, chol, u, eps)
    comp, z32, _ = raw_sample(prior.cdf, prior.means, prior.cov_chol, n, dev64(u), dev32(eps), None, 104, G.F32)
    assert np.array_equal(comp.cpu().numpy(), comp_w)
    mag = np.abs(mean[comp_w]) + np.einsum("nij,nj->ni", np.abs(np.tril(chol))[comp_w], np.abs(eps.astype(np.float64)))
    bound = 2 * (D + 2) * 2.0 ** -53 * mag + 2.0 ** -24 * np.abs(z64_w)
    assert np.all(np.abs(z32.cpu().numpy().astype(np.float64) - z64_w) <= bound)


def test_in_kernel_draws_are_the_materialised_ones(fitted):
    _, _, _, prior = fitted
    n, D = 130, 100
    ns = ops.NoiseStream(DEV, 1234)
    ns.advance()
    u = ops.rand_u01(n, ns.state, ops.DRAW_GMM_U).double()
    eps = ns.randn((n, D), ops.DRAW_GMM_EPS)
    a = raw_sample(prior.cdf, prior.means, prior.cov_chol, n, None, None, ns.state, 104, G.BF16)
    b = raw_sample(prior.cdf, prior.means, prior.cov_chol, n, u, eps, None, 104, G.BF16)
    c = raw_sample(prior.cdf, prior.means, prior.cov_chol, n, u, None, ns.state, 104, G.BF16)
    assert not torch.isnan(a[1]).any() and not torch.isnan(a[2].float()).any() and int(a[0].min()) >= 0
    for x, y, w in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, w)
    assert len(torch.unique(a[0])) > 1


def test_the_default_stream_advances_once_per_call_and_repeats(fitted):
    _, _, _, prior = fitted
    V.configure_seed(5)
    a = prior.sample(6)
    st = ops.default_noise(prior.means.device).state
    assert a.shape == (6, 100) and a.dtype == torch.float32 and int(st[1].item()) == 1
    b = prior.sample_z(6)
    assert b.shape == (6, 1, 1, G.padc(100, G.F32)) and int(st[1].item()) == 2
    assert not torch.equal(a, b.view(6, -1)[:, :100])
    prior.sample(6, torch.rand(6, dtype=torch.float64, device=DEV), torch.randn(6, 100, device=DEV))
    assert int(ops.default_noise(prior.means.device).state[1].item()) == 2                 # nothing drawn: no step
    V.configure_seed(5)
    assert torch.equal(prior.sample(6), a)
    z, comp = prior.sample_z(6, return_comp=True)
    assert torch.equal(z, b) and comp.shape == (6,)


def test_component_frequencies_follow_the_weights(fitted):
    _, _, _, prior = fitted
    n = 1 << 16
    ns = ops.NoiseStream(DEV, 77)
    ns.advance()
    comp, _, _ = ops.gmm_sample(prior.cdf, prior.means, prior.cov_chol, n, None, None, ns.state, want_comp=True,
                                want_z32=False)
    counts = np.bincount(comp.cpu().numpy(), minlength=4)
    w = prior.weights.cpu().numpy()
    assert counts.sum() == n and np.all(np.abs(counts - n * w) <= 6 * np.sqrt(n * w * (1 - w)))


# ---- 6: integration -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_evaluate_generation_with_a_mixture_prior_equals_the_loop_from_public_pieces(jpeg_folder, fitted, dtype):  # noqa: F811
    _, _, _, prior = fitted
    ds = data.ResidentImages.from_folder(jpeg_folder, device=DEV, workers=1)
    _, g, _, _ = build(64, dtype)
    vl = data.DeviceLoader(ds, torch.arange(30, 40), 4)                    # 4 + 4 + 2
    gen = torch.Generator().manual_seed(99)
    draws = [(torch.rand(b, dtype=torch.float64, generator=gen).to(DEV), torch.randn(b, 100, generator=gen).to(DEV))
             for b in (4, 4, 2)]
    calls = []

    def noise_fn(i, b):
        calls.append((i, b))
        return draws[i]
    got = V.evaluate_generation(g, vl, prior, noise_fn)
    assert calls == [(0, 4), (1, 4), (2, 2)] and not g.training
    assert got["samples"] == 10 and got["batches"] == 3 and set(got) == {"ssim", "samples", "batches"}
    tot = 0.0
    with torch.no_grad():
        for (u, eps), real in zip(draws, vl):
            b = real.shape[0]
            z = prior.sample_z(b, g, u, eps)
            fake = g(z.view(b, -1)[:, :100].float().reshape(b, 100, 1, 1).contiguous())
            tot += b * float(ops.ssim(fake, real).item())
    print("ssim", got["ssim"], "loop", tot / 10)
    assert abs(got["ssim"] - tot / 10) <= 1e-5
    V.configure_seed(3)
    r = V.evaluate_generation(g, vl, prior)
    assert math.isfinite(r["ssim"]) and -1.0 <= r["ssim"] <= 1.0 and r["samples"] == 10
    assert int(ops.default_noise(prior.means.device).state[1].item()) == 3  # one step of the stream per batch
    V.configure_seed(3)
    assert V.evaluate_generation(g, vl, prior)["ssim"] == r["ssim"]


def test_sample_images_and_the_state_dict_round_trip(fitted):
    _, xd, _, prior = fitted
    _, g, _, _ = build(64, "bf16")
    img = V.sample_images(g, n=5, prior=prior)
    assert img.shape == (5, 3, 64, 64) and img.dtype == torch.uint8 and img.is_cuda
    grid = V.sample_images(g, n=5, prior=prior, grid_cols=3)
    assert grid.shape == (2 * 64, 3 * 64, 3)
    small = V.GaussianMixturePrior.fit(dev32(R.make_mixture(600, 5, 2)), 2)
    with pytest.raises(RuntimeError, match="nz"):
        small.sample_z(4, g)
    buf = io.BytesIO()
    torch.save(prior.state_dict(), buf)
    buf.seek(0)
    sd = torch.load(buf, map_location="cpu")
    assert all(isinstance(v, torch.Tensor) for v in sd.values())
    back = V.GaussianMixturePrior.from_state_dict(sd)
    for k in ("weights", "means", "covariances", "prec_chol", "cov_chol", "cdf"):
        assert torch.equal(getattr(back, k), getattr(prior, k)) and getattr(back, k).is_cuda
    assert (back.converged, back.n_iter, back.lower_bound, back.n_fitted, back.latent_dim) == \
        (prior.converged, prior.n_iter, prior.lower_bound, prior.n_fitted, prior.latent_dim)
    u, eps = torch.rand(7, dtype=torch.float64, device=DEV), torch.randn(7, 100, device=DEV)
    assert torch.equal(back.sample(7, u, eps), prior.sample(7, u, eps))
    assert small.load_state_dict(sd).latent_dim == 100 and torch.equal(small.means, prior.means)
