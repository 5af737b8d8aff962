"""GPU: the Kernel Inception Distance (vg_kid_scores, ops.kid_scores, metrics.kernel_distance and the two evaluation
loops above them) against the f64 numpy restatement tests/_kid_ref.py on the host copy of the SAME f32 inputs.  No
expectation comes from the kernel under test.

The bound of the general cases, derived and not fitted (u = 2^-53, the unit roundoff of f64).  For one kernel value, with
Bbar_ij = |gamma| sum_c |a_c b_c| + |coef| >= |b_ij|:
  dot        the f32 x f32 products are exact in f64; D additions in whatever order: |d dot| <= D u sum_c |a_c b_c|
  affine     one multiplication by gamma and one addition of coef: |d b| <= (D + 2) u Bbar_ij
  power      degree - 1 multiplications, each rounded once, of a base off by (D + 2) u relative to Bbar:
             |d k| <= (degree (D + 2) + degree - 1) u Bbar^degree <= degree (D + 3) u Bbar^degree
  sum        n_f terms added in any order: at most (n_f - 1) u sum |k_ij| <= n_f u sum Bbar_ij^degree
so a computed sum is within E = (degree (D + 3) + n_f) u sum_ij Bbar_ij^degree of the exact one, to first order (doubling
an off-diagonal tile is exact).  The restatement is f64 arithmetic of the same class with another order of additions, so
it obeys the same E; the two can differ by 2 E, and the second-order terms ((D u)^2 and smaller) vanish beside that:
      |d sum| <= 2 (degree (D + 3) + n_f) u sum Bbar_ij^degree
  score      (s0 + s1) / (m (m - 1)) - 2 s2 / m^2: the sums' bounds through the formula, plus 4 u per term for its own
             roundings (one addition, two divisions, one subtraction, on either side).
Every test prints err / bound.  Parity with the torchmetrics package itself is unpinned: it is not installed."""
import numpy as np
import pytest
import torch

import _kid_ref as K
import vaegan_amd as V
from test_gpu_parity import build

pytestmark = pytest.mark.gpu
DEV = "cuda"
ops, M = V.ops, V.metrics
U = K.U


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def run(real, fake, ir, jf, degree, gamma, coef):
    scores, stat, sums = ops.kid_scores(dev(real), dev(fake), dev(ir), dev(jf), degree, gamma, coef)
    return scores.cpu().numpy(), stat.cpu().numpy(), sums.cpu().numpy()


def assert_within_bounds(tag, real, fake, ir, jf, degree, gamma, coef, scores, sums):
    wsc, _, _, wsums = K.kid(real, fake, ir, jf, degree, gamma, coef)
    ds, dsc = K.kid_bounds(real, fake, ir, jf, degree, gamma, coef)
    es, esc = np.abs(sums - wsums), np.abs(scores - wsc)
    print(tag, "sums err/bound", float((es / ds).max()), "scores err/bound", float((esc / dsc).max()),
          "score", float(wsc[0]), "largest sum", float(np.abs(wsums).max()))
    assert np.isfinite(sums).all() and np.isfinite(scores).all()
    assert (es <= ds).all() and (esc <= dsc).all()
    return wsc, wsums


# ---- 1: exact ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,m,D", [(300, 193, 64), (150, 130, 37)])
def test_integer_features_give_the_exact_sums(N, m, D):
    """Entries in [-3, 3], gamma = coef = 1, degree 3: every intermediate is an integer far below 2^53 (|b| <= 9 D + 1,
    sum |k| < 2^31 at these shapes), so any order of additions gives the same bits."""
    real, fake = K.int_feats(N, D, 10 + D), K.int_feats(N, D, 20 + D)
    ir, jf = K.tables(N, 3, m, 1), K.tables(N, 3, m, 2)
    wsc, _, _, wsums = K.kid(real, fake, ir, jf, 3, 1.0, 1.0)
    assert np.abs(wsums).max() < 2.0 ** 53 and (wsums == np.round(wsums)).all()
    scores, _, sums = run(real, fake, ir, jf, 3, 1.0, 1.0)
    assert np.array_equal(sums.view(np.int64), wsums.view(np.int64))
    t1, t2 = np.abs(wsums[:, 0] + wsums[:, 1]) / (m * (m - 1.0)), 2.0 * np.abs(wsums[:, 2]) / (m * m)
    print("exact: score err / (4u (t1 + t2))", float((np.abs(scores - wsc) / (4 * U * (t1 + t2))).max()))
    assert (np.abs(scores - wsc) <= 4 * U * (t1 + t2)).all()


# ---- 2: general -------------------------------------------------------------------------------------------------------
GENERAL = [(m, D) for m in (2, 63, 64, 65, 97, 200) for D in (1, 3, 37, 64, 100)] + [(65, 2048)]


@pytest.mark.parametrize("case", range(len(GENERAL)), ids=[f"m{m}-D{D}" for m, D in GENERAL])
def test_general_features_within_the_derived_bound(case):
    m, D = GENERAL[case]
    degree = 1 + case % 4
    S = 5 if (case // 4 + case) % 2 else 1
    gamma = (-0.7 if case % 3 == 0 else 1.0) / D
    coef = -0.5 if case % 5 == 0 else 1.0
    Nr, Nf = m + 37, m + 11
    real = K.gauss_feats(Nr, D, 1000 + case, mix=D <= 128)
    fake = (K.gauss_feats(Nf, D, 2000 + case, mix=D <= 128) * 0.8 + 0.25).astype(np.float32)
    ir, jf = K.tables(Nr, S, m, 3000 + case), K.tables(Nf, S, m, 4000 + case)
    scores, stat, sums = run(real, fake, ir, jf, degree, gamma, coef)
    assert_within_bounds(f"m={m} D={D} degree={degree} S={S}", real, fake, ir, jf, degree, gamma, coef, scores, sums)


# ---- 3: position, not value ---------------------------------------------------------------------------------------------
def test_pairs_are_left_out_by_position_not_by_value_or_row_index():
    """fake is real and the tables are identical, the matrix holds duplicated rows and one table row repeats an index:
    sums[2] - sums[0] is then the sum of k(x_i, x_i) over the POSITIONS only.  Leaving pairs out by zero distance or by
    row index would also drop the duplicates' cross terms."""
    N, m, D, degree, gamma, coef = 120, 70, 37, 3, 1.0 / 37, 1.0
    x = K.gauss_feats(N, D, 5)
    x[1], x[17], x[90] = x[0], x[0], x[33]                               # equal rows under different indices
    ir = np.stack([np.arange(m), np.arange(m)[::-1] + 30]).astype(np.int32)
    ir[1, 10] = ir[1, 11]                                                # and one index twice in a subset
    assert len(set(ir[0].tolist()) & {0, 1, 17}) == 3 and {33, 90} <= set(ir[1].tolist())
    xd, it = dev(x), dev(ir)
    scores, _, sums = ops.kid_scores(xd, xd, it, it, degree, gamma, coef)
    scores, sums = scores.cpu().numpy(), sums.cpu().numpy()
    ds, _ = K.kid_bounds(x, x, ir, ir, degree, gamma, coef)
    for s in range(2):
        rows = x[ir[s]].astype(np.float64)
        want = float(((gamma * (rows * rows).sum(1) + coef) ** degree).sum())
        got = sums[s, 2] - sums[s, 0]
        bound = ds[s, 0] + ds[s, 2] + U * (abs(sums[s, 0]) + abs(sums[s, 2]))
        print("position: diagonal", want, "err/bound", abs(got - want) / bound)
        assert abs(got - want) <= bound and want > 100 * bound
        assert sums[s, 0] == sums[s, 1]
    assert_within_bounds("position", x, x, ir, ir, degree, gamma, coef, scores, sums)


# ---- 4: gather and tails ------------------------------------------------------------------------------------------------
def test_only_the_tables_rows_are_read():
    """N >> m, reversed and strided tables, one repeated index; every row that no table names is NaN."""
    Nr, Nf, m, D, S = 5000, 4000, 70, 37, 3
    real, fake = K.gauss_feats(Nr, D, 8), K.gauss_feats(Nf, D, 9)
    i = np.arange(m)
    ir = np.stack([Nr - 1 - 7 * i - s for s in range(S)]).astype(np.int32)
    jf = np.stack([3 + 11 * i + 5 * s for s in range(S)]).astype(np.int32)
    jf[1, 5] = jf[1, 4]
    assert ir.min() >= 0 and jf.max() < Nf
    real[np.setdiff1d(np.arange(Nr), ir.ravel())] = np.nan
    fake[np.setdiff1d(np.arange(Nf), jf.ravel())] = np.nan
    assert np.isnan(real).any(1).sum() >= Nr - S * m and np.isnan(fake).any(1).sum() >= Nf - S * m
    scores, stat, sums = run(real, fake, ir, jf, 3, 1.0 / D, 1.0)
    assert np.isfinite(stat).all()
    assert_within_bounds("gather", real, fake, ir, jf, 3, 1.0 / D, 1.0, scores, sums)


# ---- 5: determinism and statistics ----------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits_and_stat_is_mean_and_population_std():
    Nr, Nf, m, D, S = 333, 301, 130, 100, 7
    real, fake = K.gauss_feats(Nr, D, 11), (K.gauss_feats(Nf, D, 12) * 0.9 + 0.1).astype(np.float32)
    ir, jf = K.tables(Nr, S, m, 13), K.tables(Nf, S, m, 14)
    a = ops.kid_scores(dev(real), dev(fake), dev(ir), dev(jf), 3, 1.0 / D, 1.0)
    b = ops.kid_scores(dev(real), dev(fake), dev(ir), dev(jf), 3, 1.0 / D, 1.0)
    assert all(torch.equal(p.view(torch.int64), q.view(torch.int64)) for p, q in zip(a, b))
    scores, stat = a[0].cpu().numpy(), a[1].cpu().numpy()
    mean, std = K.mean_std(scores)
    # S additions and a division on either side; the root mean square about c is 1-Lipschitz in c
    dmean = 2 * (S + 1) * U * np.abs(scores).sum() / S
    dstd = 2 * (dmean + (S + 4) * U * std)
    print("stat", stat, "numpy", mean, std, "err/bound", abs(stat[0] - mean) / dmean, abs(stat[1] - std) / dstd)
    assert abs(stat[0] - mean) <= dmean and abs(stat[1] - std) <= dstd and std > 0
    _, one, _ = ops.kid_scores(dev(real), dev(fake), dev(ir[:1]), dev(jf[:1]), 3, 1.0 / D, 1.0)
    one = one.cpu().numpy()
    assert one[1] == 0.0 and one[0] == scores[0]


def assert_mean_std(got, wsc, wmean, wstd, dsc):
    """Scores within dsc of the restatement's: their mean moves by at most max dsc, and so does their root mean square
    about the mean (1-Lipschitz in a common shift, and in the largest single perturbation); r is the rounding of the S
    additions and the division on either side."""
    S = len(wsc)
    r = 2 * (S + 1) * U * np.abs(wsc).max()
    assert abs(got["kid_mean"] - wmean) <= dsc.max() + r
    assert abs(got["kid_std"] - wstd) <= dsc.max() + 2 * r + 2 * (S + 4) * U * wstd


# ---- 6: kernel_distance ---------------------------------------------------------------------------------------------------
def test_kernel_distance_defaults_equal_the_restatement_on_its_own_draw():
    Nr, Nf, D, S, m = 400, 350, 64, 6, 150
    real, fake = K.gauss_feats(Nr, D, 21), (K.gauss_feats(Nf, D, 22) * 0.8 + 0.25).astype(np.float32)
    got, scores = M.kernel_distance(dev(real), dev(fake), subsets=S, subset_size=m, seed=3, return_scores=True)
    assert set(got) == {"kid_mean", "kid_std", "subsets", "subset_size", "feature_dim"}
    assert (got["subsets"], got["subset_size"], got["feature_dim"]) == (S, m, D)
    assert scores.is_cuda and scores.dtype == torch.float64 and tuple(scores.shape) == (S,)
    ir, jf = M.kid_subsets(Nr, Nf, S, m, 3)
    wsc, wmean, wstd, _ = K.kid(real, fake, ir, jf)                      # gamma = 1 / D, degree 3, coef 1
    _, dsc = K.kid_bounds(real, fake, ir, jf, 3, 1.0 / D, 1.0)
    esc = np.abs(scores.cpu().numpy() - wsc)
    print("kernel_distance", got, "restatement", wmean, wstd, "scores err/bound", float((esc / dsc).max()))
    assert (esc <= dsc).all()
    assert_mean_std(got, wsc, wmean, wstd, dsc)
    assert wmean > 10 * dsc.max()
    # the same tables injected (as numpy, and as a device tensor): the same bits
    again = M.kernel_distance(dev(real), dev(fake), idx_real=ir, idx_fake=dev(jf).long())
    assert again == got
    assert M.kernel_distance(dev(real), dev(fake), subsets=S, subset_size=m, seed=4)["kid_mean"] != got["kid_mean"]
    with pytest.raises(ValueError):
        M.kernel_distance(dev(real), dev(fake), subsets=2, subset_size=Nf + 1)
    with pytest.raises(ValueError):
        M.kernel_distance(dev(real), dev(fake), idx_real=ir, idx_fake=jf + Nf)
    with pytest.raises(RuntimeError):
        M.kernel_distance(dev(real), dev(fake).double(), subsets=2, subset_size=8)


# ---- 7: end to end --------------------------------------------------------------------------------------------------------
def smooth_images(n, S, seed):
    """f32 [n, 3, S, S] in [-1, 1]: low-frequency pictures with per-image colour and contrast."""
    g = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, S), np.linspace(0, 1, S), indexing="ij")
    out = np.empty((n, 3, S, S), np.float32)
    for i in range(n):
        for c in range(3):
            f, ph = g.uniform(0.5, 4.0, 2), g.uniform(0, 6.28, 2)
            out[i, c] = g.uniform(0.2, 0.9) * np.sin(6.28 * f[0] * yy + ph[0]) * np.cos(6.28 * f[1] * xx + ph[1]) + g.uniform(-0.1, 0.1)
    return torch.from_numpy(np.clip(out, -1, 1))


class Capture:
    def __init__(self, fn):
        self.fn, self.out = fn, []

    def __call__(self, u8):
        f = self.fn(u8)
        self.out.append(f.cpu().numpy().copy())
        return f


def assert_kid_keys(got, real, fake, S, m, seed):
    D = real.shape[1]
    ir, jf = M.kid_subsets(len(real), len(fake), S, m, seed)
    _, dsc = K.kid_bounds(real, fake, ir, jf, 3, 1.0 / D, 1.0)
    wsc, wmean, wstd, _ = K.kid(real, fake, ir, jf)
    print("e2e kid", got["kid_mean"], got["kid_std"], "restatement", wmean, wstd, "bound", dsc.max())
    assert_mean_std(got, wsc, wmean, wstd, dsc)


def test_evaluate_generation_with_kid_end_to_end():
    e, g, _, _ = build(64)
    vl = [t.to(DEV) for t in torch.split(smooth_images(16, 64, 31), 8)]
    gen = torch.Generator().manual_seed(7)
    zs = [torch.randn(8, 100, generator=gen).to(DEV) for _ in vl]
    plain = V.evaluate_generation(g, vl, None, lambda i, b: zs[i])
    assert set(plain) == {"ssim", "samples", "batches"}
    base = V.evaluate_generation(g, vl, None, lambda i, b: zs[i], feature_fn=M.encoder_features(e))
    assert set(base) == {"ssim", "samples", "batches", "fid", "precision", "recall", "f1", "feature_dim"}
    cap = Capture(M.encoder_features(e))
    got = V.evaluate_generation(g, vl, None, lambda i, b: zs[i], feature_fn=cap, kid_subsets=4, kid_subset_size=8, kid_seed=1)
    assert set(got) == set(base) | {"kid_mean", "kid_std"}
    assert all(got[key] == base[key] for key in base)
    assert_kid_keys(got, np.concatenate(cap.out[0::2]), np.concatenate(cap.out[1::2]), 4, 8, 1)
    with pytest.raises(RuntimeError, match="feature_fn"):
        V.evaluate_generation(g, vl, None, lambda i, b: zs[i], kid_subsets=4, kid_subset_size=8)


def test_validation_epoch_with_kid_end_to_end():
    e, g, _, _ = build(64)
    vl = [t.to(DEV) for t in torch.split(smooth_images(16, 64, 32), 8)]
    gen = torch.Generator().manual_seed(8)
    noises = [(torch.randn(8, 3, 64, 64, generator=gen).to(DEV), torch.randn(8, 100, generator=gen).to(DEV)) for _ in vl]
    plain = V.validation_epoch(e, g, vl, noise_fn=lambda i, img: noises[i])
    assert set(plain) == {"val_loss", "ssim", "psnr", "recon_loss", "kl_loss", "samples", "batches"}
    base = V.validation_epoch(e, g, vl, noise_fn=lambda i, img: noises[i], feature_fn=M.encoder_features(e))
    assert set(base) == set(plain) | {"fid"}
    cap = Capture(M.encoder_features(e))
    got = V.validation_epoch(e, g, vl, noise_fn=lambda i, img: noises[i], feature_fn=cap, kid_subsets=4, kid_subset_size=8,
                             kid_seed=1)
    assert set(got) == set(base) | {"kid_mean", "kid_std"}
    assert all(got[key] == base[key] for key in base)
    assert_kid_keys(got, np.concatenate(cap.out[0::2]), np.concatenate(cap.out[1::2]), 4, 8, 1)
    with pytest.raises(RuntimeError, match="feature_fn"):
        V.validation_epoch(e, g, vl, noise_fn=lambda i, img: noises[i], kid_subsets=4)
