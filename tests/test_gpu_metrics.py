"""GPU: the feature-space metrics (vg_feat_stats_accum, vg_knn_radius2, vg_manifold_cover, metrics.py and the evaluation
loops above them) against the f64 numpy restatement tests/_metrics_ref.py on the host copy of the SAME f32 inputs.  No
expectation comes from a kernel under test.  Bounds (derived, not measured):
  statistics   only the order of the f64 additions differs (f32 x f32 is exact in f64): |err_ij| <= n 2^-52 sum_r |x_ri x_rj|
  FID          through |sqrt(l + d) - sqrt(l)| <= sqrt(d): 2 D sqrt(eps |S1| |S2|), eps = n 2^-52 the relative bound above
  distances    the standard f32 dot-product bound: tol_ij = 2 (D + 4) 2^-24 (|a_i|^2 + |b_j|^2); the k-th order statistic is
               1-Lipschitz in the row's perturbation, so a radius is off by at most tol_i = max_j tol_ij
  decisions    a sample is DECIDED in f64 when it is inside by more than 2 tol for some j or outside by more than 2 tol for
               every j; every decided flag must match, precision / recall may differ by at most undecided / N.
Parity with the torchmetrics package itself is unpinned: it is not installed."""
import numpy as np
import pytest
import torch

import _metrics_ref as R
import vaegan_amd as V
from test_gpu_parity import build

pytestmark = pytest.mark.gpu
DEV = "cuda"
ops, M = V.ops, V.metrics
U52 = 2.0 ** -52


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def feats(n, D, seed, mix=True):
    """f32 [n, D]: correlated Gaussian columns of mixed scale with offsets (full rank for n >= D)."""
    g = np.random.default_rng(seed)
    x = g.standard_normal((n, D))
    if mix and D > 1:
        x = x @ (np.eye(D) + 0.3 * g.standard_normal((D, D)) / np.sqrt(D))
    return (x * g.uniform(0.5, 2.0, D) + g.uniform(-1, 1, D)).astype(np.float32)


def fresh(D):
    return torch.zeros(D, dtype=torch.float64, device=DEV), torch.zeros(D, D, dtype=torch.float64, device=DEV)


def assert_stats_close(s, o, x, n_bound, base=None):
    """(s, o) against numpy f64 on x, |err| <= n_bound 2^-52 sum_r |.| (elementwise)."""
    x64 = x.astype(np.float64)
    ws, wo, _ = R.stats(x64)
    if base is not None:
        ws, wo = ws + base[0], wo + base[1]
    ab = np.abs(x64)
    bs, bo = n_bound * U52 * ab.sum(0), n_bound * U52 * (ab.T @ ab)
    if base is not None:
        bs, bo = bs + U52 * np.abs(ws), bo + U52 * np.abs(wo)           # the one addition to the value already there
    es, eo = np.abs(s.cpu().numpy() - ws), np.abs(o.cpu().numpy() - wo)
    print("stats err/bound: sum", float((es / np.maximum(bs, 1e-300)).max()) if es.size else 0.0,
          "outer", float((eo / np.maximum(bo, 1e-300)).max()) if eo.size else 0.0)
    assert (es <= bs).all() and (eo <= bo).all()


# ---- 1: f64 running statistics ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 37, 64, 100, 2048])
@pytest.mark.parametrize("n", [0, 1, 13, 4099])
def test_feat_stats_accum_equals_numpy_f64(n, D):
    x = feats(n, D, 100 * D + n, mix=D <= 128)
    s, o = fresh(D)
    ops.feat_stats_accum(dev(x) if n else torch.empty(0, D, dtype=torch.float32, device=DEV), s, o)
    if n == 0:
        assert not s.any() and not o.any()
        return
    assert_stats_close(s, o, x, n)
    assert torch.equal(o, o.T)                                          # the full symmetric matrix
    s2, o2 = fresh(D)
    ops.feat_stats_accum(dev(x), s2, o2)
    assert torch.equal(s, s2) and torch.equal(o, o2)                    # deterministic: bitwise


def test_feat_stats_accum_strided_rows_and_accumulation():
    full = feats(3000, 160, 5)
    view = dev(full)[:, 8:108]                                          # rows 160 apart, 100 columns
    assert not view.is_contiguous()
    s, o = fresh(100)
    ops.feat_stats_accum(view, s, o)
    x = np.ascontiguousarray(full[:, 8:108])
    assert_stats_close(s, o, x, 3000)
    # += : a second call adds to what is there
    y = feats(777, 100, 6)
    base = (s.cpu().numpy().copy(), o.cpu().numpy().copy())
    ops.feat_stats_accum(dev(y), s, o)
    assert_stats_close(s, o, y, 777, base=base)


def test_feature_stats_ragged_updates_equal_one_update():
    D, n = 100, 4099
    x = feats(n, D, 7)
    xd = dev(x)
    one = M.FeatureStats(D, DEV).update(xd)
    three = M.FeatureStats(D, DEV)
    for lo, hi in ((0, 1500), (1500, 1501), (1501, n)):
        three.update(xd[lo:hi])
    three.update(xd[:0])                                                # an empty batch is a no-op
    assert one.n == three.n == n
    assert_stats_close(one.sum, one.outer, x, n)
    assert_stats_close(three.sum, three.outer, x, n)
    again = M.FeatureStats(D, DEV).update(xd)
    assert torch.equal(again.outer, one.outer) and torch.equal(again.sum, one.sum)
    m, c = R.mean_cov(*R.stats(x))
    assert np.allclose(one.mean(), m, rtol=1e-12, atol=1e-14) and np.allclose(one.cov(), c, rtol=1e-9, atol=1e-12)
    both = M.FeatureStats(D, DEV).update(xd[:2000]).merge(M.FeatureStats(D, DEV).update(xd[2000:]))
    assert both.n == n
    assert_stats_close(both.sum, both.outer, x, n)
    with pytest.raises(RuntimeError):
        one.update(xd[:, :50])
    with pytest.raises(RuntimeError):
        one.update(xd.double())


# ---- 2: FID -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,N", [(64, 3000), (100, 1000), (37, 512)])
def test_frechet_distance_from_device_statistics(D, N):
    assert N >= 8 * D
    real, fake = feats(N, D, 11 * D), (feats(N + 5, D, 13 * D) * 0.8 + 0.25).astype(np.float32)
    a = M.FeatureStats(D, DEV).update(dev(real))
    b = M.FeatureStats(D, DEV)
    for lo in range(0, N + 5, 300):                                     # ragged: the last batch is short
        b.update(dev(fake)[lo:lo + 300])
    got = M.frechet_distance(a, b)
    want = R.fid(real, fake)
    _, c1 = R.mean_cov(*R.stats(real))
    _, c2 = R.mean_cov(*R.stats(fake))
    eps = (N + 5) * U52
    bound = 2.0 * D * np.sqrt(eps * np.linalg.norm(c1, 2) * np.linalg.norm(c2, 2))
    print("fid", got, "restatement", want, "err", abs(got - want), "bound", bound)
    assert want > 0 and abs(got - want) <= bound
    # saved real statistics give the same number
    saved = {k: v.cpu() for k, v in a.state_dict().items()}
    assert M.frechet_distance(M.FeatureStats(D, DEV).load_state_dict(saved), b) == got
    assert M.frechet_distance(a, a) <= bound


# ---- 3: k-th neighbour radius -------------------------------------------------------------------------------------------
def radius_tol(x):
    n2 = (x.astype(np.float64) ** 2).sum(1)
    return 2.0 * (x.shape[1] + 4) * 2.0 ** -24 * (n2 + n2.max())        # tol_i = max_j tol_ij


@pytest.mark.parametrize("N,D,k", [(1000, 64, 3), (777, 37, 1), (513, 3, 8), (2048, 100, 3), (130, 64, 8), (129, 100, 1),
                                   (9, 5, 8), (1500, 200, 3)])
def test_knn_radius2_equals_brute_force(N, D, k):
    x = feats(N, D, N + D + k)
    got = ops.knn_radius2(dev(x), k).cpu().numpy().astype(np.float64)
    want = R.knn_radius2(x, k)
    err, tol = np.abs(got - want), radius_tol(x)
    print("knn err/tol", float((err / tol).max()))
    assert (err <= tol).all()
    again = ops.knn_radius2(dev(x), k).cpu().numpy()
    assert np.array_equal(again.astype(np.float64), got)                # deterministic


def test_knn_radius2_duplicated_rows_and_views():
    x = feats(300, 37, 3)
    x[7], x[150], x[299] = x[8], x[8], x[0]                             # rows 7, 8, 150 equal; 0 and 299 equal
    got = ops.knn_radius2(dev(x), 1).cpu().numpy().astype(np.float64)
    want = R.knn_radius2(x, 1)
    assert (want[[0, 7, 8, 150, 299]] == 0).all() and (np.delete(want, [0, 7, 8, 150, 299]) > 0).all()
    assert (np.abs(got - want) <= radius_tol(x)).all()                  # a row is left out by index, its duplicate counts
    got2 = ops.knn_radius2(dev(x), 2).cpu().numpy().astype(np.float64)
    assert (np.abs(got2 - R.knn_radius2(x, 2)) <= radius_tol(x)).all() and got2[0] > 0 and abs(got2[8]) <= radius_tol(x)[8]
    # a view that starts off the 16-byte grid, and one with a row stride
    xd = dev(x)
    assert (np.abs(ops.knn_radius2(xd[1:], 3).cpu().numpy() - R.knn_radius2(x[1:], 3)) <= radius_tol(x[1:])).all()
    sub = np.ascontiguousarray(x[:, 4:20])
    assert (np.abs(ops.knn_radius2(xd[:, 4:20], 3).cpu().numpy() - R.knn_radius2(sub, 3)) <= radius_tol(sub)).all()
    with pytest.raises(RuntimeError):
        ops.knn_radius2(xd, 9)
    with pytest.raises(RuntimeError):
        ops.knn_radius2(xd[:3], 3)


@pytest.mark.parametrize("N,D,k", [(517, 37, 3), (300, 64, 8), (1000, 100, 1)])
def test_knn_radius2_is_exact_on_small_integers(N, D, k):
    """Entries in [-3, 3]: every norm, dot product and difference is an integer below 2^24, so f32 is exact."""
    x = np.random.default_rng(N).integers(-3, 4, (N, D)).astype(np.float32)
    got = ops.knn_radius2(dev(x), k).cpu().numpy()
    want = R.knn_radius2(x, k).astype(np.float32)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


# ---- 4: manifold cover, precision / recall ----------------------------------------------------------------------------
PR_CASES = [(2048, 2048, 64, 0.35, 0.9), (2048, 2048, 100, 0.2, 0.95), (1000, 1000, 64, 0.0, 1.0), (1500, 1000, 64, 0.35, 0.9),
            (700, 1300, 37, 0.3, 0.9)]


def pr_sets(Nr, Nf, D, shift, scale):
    g = np.random.default_rng(7)
    real = g.standard_normal((Nr, D)).astype(np.float32)
    fake = (shift + scale * g.standard_normal((Nf, D))).astype(np.float32)
    return real, fake


@pytest.mark.parametrize("Nr,Nf,D,shift,scale", PR_CASES)
def test_manifold_cover_and_precision_recall(Nr, Nf, D, shift, scale):
    k = 3
    real, fake = pr_sets(Nr, Nf, D, shift, scale)
    r2_real, r2_fake = R.knn_radius2(real, k), R.knn_radius2(fake, k)
    in_p, dec_p = R.decided_cover(fake, real, r2_real)                  # precision side: fake rows in the real manifold
    in_r, dec_r = R.decided_cover(real, fake, r2_fake)                  # recall side
    und_p, und_r = int((~dec_p).sum()), int((~dec_r).sum())
    print("reference precision", in_p.mean(), "recall", in_r.mean(), "undecided", und_p, und_r)
    assert und_p <= 0.01 * Nf and und_r <= 0.01 * Nr                    # condition on the inputs, before the device is asked
    rd, fd = dev(real), dev(fake)
    # the cover kernel alone, radii computed on the device
    inside, count = ops.manifold_cover(fd, rd, ops.knn_radius2(rd, k))
    inside = inside.cpu().numpy()
    assert set(np.unique(inside)) <= {0, 1} and int(count.item()) == int(inside.sum())
    assert np.array_equal(inside[dec_p].astype(bool), in_p[dec_p])
    inside_r, count_r = ops.manifold_cover(rd, fd, ops.knn_radius2(fd, k))
    assert np.array_equal(inside_r.cpu().numpy()[dec_r].astype(bool), in_r[dec_r])
    assert int(count_r.item()) == int(inside_r.sum().item())
    # radii handed in from the host: the same decisions
    inside_h, _ = ops.manifold_cover(fd, rd, dev(r2_real.astype(np.float32)))
    assert np.array_equal(inside_h.cpu().numpy()[dec_p].astype(bool), in_p[dec_p])
    # the public function
    got = M.precision_recall(rd, fd, k)
    want = R.precision_recall(real, fake, k)
    print("device", got, "restatement", want)
    assert abs(got["precision"] - want["precision"]) <= und_p / Nf
    assert abs(got["recall"] - want["recall"]) <= und_r / Nr
    assert got["precision"] == count.item() / Nf and got["recall"] == count_r.item() / Nr
    p, r = got["precision"], got["recall"]
    assert got["f1"] == (0.0 if p + r == 0 else 2 * p * r / (p + r))
    assert (got["n_real"], got["n_fake"], got["k"]) == (Nr, Nf, k)
    assert M.precision_recall(rd, fd, k) == got                         # deterministic


def test_precision_recall_closed_forms_on_the_device():
    x = feats(400, 32, 1, mix=False)
    r = M.precision_recall(dev(x), dev(x.copy()), 3)
    assert r["precision"] == 1.0 and r["recall"] == 1.0 and r["f1"] == 1.0
    far = (feats(300, 32, 2, mix=False) + 1000.0).astype(np.float32)
    r = M.precision_recall(dev(x), dev(far), 3)
    assert r["precision"] == 0.0 and r["recall"] == 0.0 and r["f1"] == 0.0
    with pytest.raises(RuntimeError):
        M.precision_recall(dev(x), dev(x[:, :8]))
    with pytest.raises(RuntimeError):
        ops.manifold_cover(dev(x), dev(x), dev(np.zeros(5, np.float32)))


def test_workspace_never_holds_the_distance_matrix():
    lib = import_lib()
    N, D, k = 30000, 2048, 3
    assert 0 < lib.vg_knn_radius2_ws_bytes(N, D, k) < 64 << 20
    assert 0 < lib.vg_manifold_cover_ws_bytes(N, N, D) < 64 << 20
    assert lib.vg_knn_radius2_ws_bytes(N, D, k) < N * N * 4 // 100


def import_lib():
    from importlib import import_module
    return import_module("vae-gan-based-model-for-image-generation-and-denoising_amd._lib").load()


# ---- 5: end to end --------------------------------------------------------------------------------------------------------
def smooth_images(n, S, seed):
    """f32 [n, 3, S, S] in [-1, 1]: low-frequency pictures with per-image colour and contrast."""
    g = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, S), np.linspace(0, 1, S), indexing="ij")
    out = np.empty((n, 3, S, S), np.float32)
    for i in range(n):
        for c in range(3):
            f = g.uniform(0.5, 4.0, 2)
            ph = g.uniform(0, 6.28, 2)
            out[i, c] = g.uniform(0.2, 0.9) * np.sin(6.28 * f[0] * yy + ph[0]) * np.cos(6.28 * f[1] * xx + ph[1]) + g.uniform(-0.1, 0.1)
    return torch.from_numpy(np.clip(out, -1, 1))


class Capture:
    def __init__(self, fn):
        self.fn, self.out = fn, []

    def __call__(self, u8):
        assert u8.dtype == torch.uint8 and u8.is_cuda and u8.dim() == 4
        f = self.fn(u8)
        self.out.append(f.cpu().numpy().copy())
        return f


def fid_bound(real, fake):
    _, c1 = R.mean_cov(*R.stats(real))
    _, c2 = R.mean_cov(*R.stats(fake))
    D = real.shape[1]
    return 2.0 * D * np.sqrt(max(len(real), len(fake)) * U52 * np.linalg.norm(c1, 2) * np.linalg.norm(c2, 2))


def test_evaluate_generation_with_features_end_to_end():
    e, g, _, _ = build(64)
    sizes = (64, 64, 37)                                                # a ragged last batch
    imgs = smooth_images(sum(sizes), 64, 21)
    vl = [t.to(DEV) for t in torch.split(imgs, sizes)]
    gen = torch.Generator().manual_seed(5)
    zs = [torch.randn(b, 100, generator=gen).to(DEV) for b in sizes]
    plain = V.evaluate_generation(g, vl, None, lambda i, b: zs[i])
    assert set(plain) == {"ssim", "samples", "batches"}                 # the default is untouched
    cap = Capture(M.encoder_features(e))
    got = V.evaluate_generation(g, vl, None, lambda i, b: zs[i], feature_fn=cap, k=3)
    assert set(got) == {"ssim", "samples", "batches", "fid", "precision", "recall", "f1", "feature_dim"}
    assert got["ssim"] == plain["ssim"] and got["samples"] == 165 and got["batches"] == 3 and got["feature_dim"] == 100
    assert not e.training and not g.training
    assert [f.shape for f in cap.out] == [(b, 100) for b in sizes for _ in (0, 1)]
    real, fake = np.concatenate(cap.out[0::2]), np.concatenate(cap.out[1::2])
    want_fid, bound = R.fid(real, fake), fid_bound(real, fake)
    print("e2e fid", got["fid"], "restatement", want_fid, "bound", bound)
    assert np.isfinite(got["fid"]) and abs(got["fid"] - want_fid) <= bound
    k = 3
    in_p, dec_p = R.decided_cover(fake, real, R.knn_radius2(real, k))
    in_r, dec_r = R.decided_cover(real, fake, R.knn_radius2(fake, k))
    print("e2e precision", got["precision"], in_p.mean(), "recall", got["recall"], in_r.mean(), "undecided",
          int((~dec_p).sum()), int((~dec_r).sum()))
    assert abs(got["precision"] - in_p.mean()) <= (~dec_p).sum() / len(fake) + 1e-15
    assert abs(got["recall"] - in_r.mean()) <= (~dec_r).sum() / len(real) + 1e-15
    p, r = got["precision"], got["recall"]
    assert got["f1"] == (0.0 if p + r == 0 else 2 * p * r / (p + r))
    # the features are the eval-mode Encoder's mu of the uint8 picture
    with torch.no_grad():
        u8 = ops.to_u8(vl[2])
        mu, _ = e((u8.float() / 255.0 - 0.5) / 0.5)
    assert np.allclose(cap.out[4], mu.cpu().numpy(), rtol=1e-4, atol=1e-5)
    assert M.encoder_features(e, "mulv")(u8).shape == (37, 200)
    # real statistics computed once and handed in: the same FID up to the bound, the real half is not accumulated again
    rs = M.FeatureStats(100, DEV)
    for f in cap.out[0::2]:
        rs.update(dev(f))
    again = V.evaluate_generation(g, vl, None, lambda i, b: zs[i], feature_fn=M.encoder_features(e), real_stats=rs)
    assert rs.n == 165 and abs(again["fid"] - want_fid) <= bound and again["precision"] == got["precision"]


def test_validation_epoch_with_features_end_to_end():
    e, g, _, _ = build(64)
    sizes = (48, 48, 21)
    imgs = smooth_images(sum(sizes), 64, 22)
    vl = [t.to(DEV) for t in torch.split(imgs, sizes)]
    gen = torch.Generator().manual_seed(6)
    noises = [(torch.randn(b, 3, 64, 64, generator=gen).to(DEV), torch.randn(b, 100, generator=gen).to(DEV)) for b in sizes]
    plain = V.validation_epoch(e, g, vl, noise_fn=lambda i, img: noises[i])
    assert "fid" not in plain
    cap = Capture(M.encoder_features(e))
    got = V.validation_epoch(e, g, vl, noise_fn=lambda i, img: noises[i], feature_fn=cap)
    assert set(got) == set(plain) | {"fid"}
    assert all(got[key] == plain[key] for key in plain)
    clean, recon = np.concatenate(cap.out[0::2]), np.concatenate(cap.out[1::2])
    want, bound = R.fid(clean, recon), fid_bound(clean, recon)
    print("validation fid", got["fid"], "restatement", want, "bound", bound)
    assert np.isfinite(got["fid"]) and abs(got["fid"] - want) <= bound
