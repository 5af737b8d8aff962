"""GPU: the latent prior (vg_latent_hist, vg_latent_sample, vg_to_u8 and latent.py above them) against the reference's own
vals_to_hist / sample_distribution output (tests/golden/latent_prior.npz), numpy on the host copy, f64 restatements and
torch on the host.  No expectation is taken from the kernel under test; bounds are those of the contract text in
include/vaegan_hip.h ("Latent prior") and of the number formats."""
import math
import os

import numpy as np
import pytest
import torch

import vaegan_amd as V
from test_gpu_data import jpeg_folder  # noqa: F401  (fixture: 45 generated 64 x 64 JPEGs)
from test_gpu_parity import build

pytestmark = pytest.mark.gpu
DEV = "cuda"
ops, data, G = V.ops, V.data, V.geometry
DRAW_U, DRAW_V, DRAW_EPS = 32, 33, 34                  # the header's VG_DRAW_LATENT_U / _V / _EPS


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "latent_prior.npz"))


def matrix(N, D, seed):
    """f32 [N, D]: Gaussian columns over four decades of scale with offsets, every fifth column rounded to quarters of
    its scale (ties, values on bin edges), column 3 constant."""
    g = np.random.default_rng(seed)
    scale = 10.0 ** g.uniform(-2, 2, D)
    x = g.standard_normal((N, D)) * scale + g.uniform(-5, 5, D) * scale
    x[:, ::5] = np.round(x[:, ::5] / scale[::5] * 4) / 4 * scale[::5]
    if D > 3:
        x[:, 3] = -2.5
    return x.astype(np.float32)


def numpy_hist(x, n_bins):
    """What vals_to_hist computes per column, by numpy itself (edges stay f32, numpy >= 2)."""
    N, D = x.shape
    edges = np.empty((D, n_bins + 1), np.float32)
    counts = np.empty((D, n_bins), np.int64)
    cdf = np.empty((D, n_bins), np.float64)
    for c in range(D):
        freqs, bins = np.histogram(x[:, c], bins=n_bins)
        assert bins.dtype == np.float32
        edges[c], counts[c], cdf[c] = bins, freqs, np.cumsum(freqs / N)
    return edges, counts, cdf


def assert_hist_equal(got, want, N):
    edges, counts, cdf, status = got
    assert int(status.item()) == 0
    assert edges.dtype == torch.float32 and counts.dtype == torch.int32 and cdf.dtype == torch.float64
    assert np.array_equal(edges.cpu().numpy().view(np.int32), want[0].view(np.int32))
    assert np.array_equal(counts.cpu().numpy().astype(np.int64), want[1])
    assert np.array_equal(cdf.cpu().numpy().view(np.int64), want[2].view(np.int64))
    assert (counts.sum(1) == N).all()


# ---- 1: the fixture ----------------------------------------------------------------------------------------------------
def test_hist_equals_the_reference_on_the_fixture_bitwise(fx):
    x, nb = fx["x"], int(fx["n_bins"])
    edges, counts, cdf, status = ops.latent_hist(torch.from_numpy(x).to(DEV), nb)
    assert int(status.item()) == 0
    assert np.array_equal(edges.cpu().numpy().astype(np.float64), fx["bins"])          # widened exactly
    assert np.array_equal(cdf.cpu().numpy().view(np.int64), fx["cdf"].view(np.int64))
    for c in range(x.shape[1]):
        assert np.array_equal(counts[c].cpu().numpy(), np.histogram(x[:, c], bins=nb)[0])
    assert (counts.sum(1) == x.shape[0]).all()


# ---- 2: sizes the fixture is too small for ------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,n_bins", [(30000, 200, 100), (1, 5, 100), (257, 1, 100), (4000, 333, 100),
                                        (5000, 20, 1), (5000, 20, 7), (5000, 20, 1024), (63, 70, 100)])
def test_hist_equals_numpy_on_generated_matrices(N, D, n_bins):
    x = matrix(N, D, 1000 * n_bins + D)
    assert_hist_equal(ops.latent_hist(torch.from_numpy(x).to(DEV), n_bins), numpy_hist(x, n_bins), N)


def test_hist_of_a_strided_view_equals_numpy():
    full = matrix(3000, 64, 9)
    dev = torch.from_numpy(full).to(DEV)
    view = dev[:, 8:40]                                                    # rows 64 floats apart, 32 columns, offset base
    assert not view.is_contiguous()
    assert_hist_equal(ops.latent_hist(view, 100), numpy_hist(np.ascontiguousarray(full[:, 8:40]), 100), 3000)
    # the [N, 2L] latents in one call are the two reference calls side by side
    both = numpy_hist(full, 100)
    mu, lv = numpy_hist(np.ascontiguousarray(full[:, :32]), 100), numpy_hist(np.ascontiguousarray(full[:, 32:]), 100)
    for k in range(3):
        assert np.array_equal(both[k], np.concatenate([mu[k], lv[k]]))


# ---- 3: non-finite input ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_fit_raises_on_a_non_finite_latent(bad):
    x = torch.from_numpy(matrix(5000, 12, 3)).to(DEV)
    assert V.LatentPrior.fit(x, 6).n_fitted == 5000
    x[4321, 7] = bad
    assert int(ops.latent_hist(x, 100)[3].item()) != 0
    with pytest.raises(RuntimeError, match="not finite"):
        V.LatentPrior.fit(x, 6)
    with pytest.raises(RuntimeError):
        V.LatentPrior.fit(x, 5)                                            # 12 columns are not 2 * 5


# ---- 4: sampling with the reference's own draws -------------------------------------------------------------------------
def test_sample_equals_the_reference_on_its_own_draws_bitwise(fx):
    D = fx["x"].shape[1]
    L = D // 2
    edges = torch.from_numpy(fx["bins"].astype(np.float32)).to(DEV)
    cdf = torch.from_numpy(fx["cdf"]).to(DEV)
    u, v = torch.from_numpy(fx["u"]).to(DEV), torch.from_numpy(fx["v"]).to(DEV)
    mulv, z = ops.latent_sample(edges, cdf, L, 40, u, v)
    assert z is None
    assert np.array_equal(mulv.cpu().numpy().view(np.int32), fx["samples"].view(np.int32))
    # through the fitted object
    prior = V.LatentPrior.fit(torch.from_numpy(fx["x"]).to(DEV), L, int(fx["n_bins"]))
    mu, lv = prior.sample(40, u, v)
    assert mu.shape == lv.shape == (40, L)
    assert np.array_equal(torch.cat([mu, lv], 1).cpu().numpy().view(np.int32), fx["samples"].view(np.int32))
    # the stated deviation: u above cdf[-1] takes the last bin instead of indexing past the edges
    nb = int(fx["n_bins"])
    assert (fx["cdf"][:, -1] < 1.0).any()
    top, _ = ops.latent_sample(edges, cdf, L, 1, torch.ones(1, D, dtype=torch.float64, device=DEV),
                               torch.full((1, D), 0.5, dtype=torch.float64, device=DEV))
    raw = np.array([np.searchsorted(fx["cdf"][c], 1.0) for c in range(D)])     # nb where cdf[-1] < 1: the reference raises
    assert (raw[fx["cdf"][:, -1] < 1.0] == nb).all() and raw[0] < nb - 1        # (constant column: full at its middle bin)
    idx = np.minimum(raw, nb - 1)
    x0, x1 = fx["bins"][np.arange(D), idx], fx["bins"][np.arange(D), idx + 1]
    assert np.array_equal(top.cpu().numpy()[0], (x0 + (x1 - x0) * 0.5).astype(np.float32))


# ---- 5: device draws ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [G.F32, G.BF16])
def test_in_kernel_draws_equal_the_materialised_draws_fed_back(dtype):
    L, n = 100, 257
    prior = V.LatentPrior.fit(torch.from_numpy(matrix(6000, 2 * L, 21)).to(DEV), L)
    ns = ops.NoiseStream(DEV, 1234)
    for _ in range(3):
        ns.advance()
    u = ops.rand_u01(n * 2 * L, ns.state, DRAW_U).double().view(n, 2 * L)
    v = ops.rand_u01(n * 2 * L, ns.state, DRAW_V).double().view(n, 2 * L)
    eps = ns.randn((n, L), DRAW_EPS)
    zspec = (G.padc(L, dtype), dtype)
    m_inj, z_inj = ops.latent_sample(prior.edges, prior.cdf, L, n, u, v, eps, None, z=zspec)
    m_dev, z_dev = ops.latent_sample(prior.edges, prior.cdf, L, n, None, None, None, ns.state, z=zspec)
    assert torch.equal(m_inj, m_dev) and torch.equal(z_inj, z_dev)
    assert z_dev.shape == (n, 1, 1, zspec[0]) and z_dev.dtype == ops.TORCH_DT[dtype]
    # injected uniforms with a drawn eps: the same again
    _, z_mix = ops.latent_sample(prior.edges, prior.cdf, L, n, u, v, None, ns.state, z=zspec)
    assert torch.equal(z_mix, z_dev)


def test_the_default_stream_advances_and_configure_seed_repeats_it():
    L = 6
    prior = V.LatentPrior.fit(torch.from_numpy(matrix(2000, 2 * L, 4)).to(DEV), L)
    V.configure_seed(5)
    a = torch.cat(prior.sample(64), 1)
    za = prior.sample_z(64)
    b = torch.cat(prior.sample(64), 1)
    assert not torch.equal(a, b)
    V.configure_seed(5)
    a2 = torch.cat(prior.sample(64), 1)
    za2 = prior.sample_z(64)
    assert torch.equal(a, a2) and torch.equal(za, za2)
    assert int(ops.default_noise(prior.edges.device).state[1].item()) == 2  # one step per call


# ---- 6: z ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [6, 100])
@pytest.mark.parametrize("dtype", [G.F32, G.BF16])
def test_z_equals_the_f64_reparameterisation_of_the_sampled_latents(L, dtype):
    g = np.random.default_rng(L)
    x = g.standard_normal((3000, 2 * L)).astype(np.float32)
    x[:, L:] = x[:, L:] * 4.0 - 1.0                                        # logvar beyond +-10 on both sides: the clamp acts
    assert x[:, L:].min() < -10 and x[:, L:].max() > 10
    prior = V.LatentPrior.fit(torch.from_numpy(x).to(DEV), L)
    n = 500
    gen = torch.Generator().manual_seed(L + dtype)
    u = torch.rand(n, 2 * L, dtype=torch.float64, generator=gen).to(DEV)
    v = torch.rand(n, 2 * L, dtype=torch.float64, generator=gen).to(DEV)
    eps = torch.randn(n, L, generator=gen).to(DEV)
    ZP = G.padc(L, dtype)
    mulv, z = ops.latent_sample(prior.edges, prior.cdf, L, n, u, v, eps, None, z=(ZP, dtype))
    m = mulv.cpu().double()
    assert (m[:, L:].abs() > 10).any()
    want = m[:, :L] + torch.exp(0.5 * m[:, L:].clamp(-10, 10)) * eps.cpu().double()
    got = z.cpu().double().view(n, ZP)
    rtol = 1e-5 if dtype == G.F32 else 2.0 ** -8
    torch.testing.assert_close(got[:, :L], want, rtol=rtol, atol=1e-5)
    if ZP > L:
        assert (z.view(n, ZP)[:, L:] == 0).all()
    else:
        assert (dtype, L) == (G.F32, 100)                                  # the one case without pad columns
    # the object's route gives the same tensor
    class _Dec:
        _dt, nz = dtype, L
    z2, mulv2 = prior.sample_z(n, _Dec, u, v, eps, return_mulv=True)
    assert torch.equal(z2, z) and torch.equal(mulv2, mulv)
    _Dec.nz = L + 1
    with pytest.raises(RuntimeError):
        prior.sample_z(n, _Dec, u, v, eps)


# ---- 7: distribution ----------------------------------------------------------------------------------------------------
def test_device_draws_follow_the_fitted_histogram():
    """200 000 draws, 200 columns x 100 bins: per bin, the share of draws within 6 binomial standard deviations of
    p = counts / N (+ 1e-5 for the few draws whose final f32 rounding lands on the bin's upper edge); none outside [lo, hi]."""
    L, N, n = 100, 5000, 200000
    g = np.random.default_rng(77)
    x = (g.standard_normal((N, 2 * L)) * g.uniform(0.5, 3.0, 2 * L) + g.uniform(-2, 2, 2 * L)).astype(np.float32)
    prior = V.LatentPrior.fit(torch.from_numpy(x).to(DEV), L)
    V.configure_seed(11)
    mu, lv = prior.sample(n)
    draws = torch.cat([mu, lv], 1).cpu().numpy()
    edges = prior.edges.cpu().numpy().astype(np.float64)
    p_all = prior.counts.cpu().numpy() / N
    assert np.array_equal(prior.counts.cpu().numpy(), numpy_hist(x, 100)[1])
    worst = 0.0
    for c in range(2 * L):
        assert edges[c, 0] <= draws[:, c].min() and draws[:, c].max() <= edges[c, -1], c
        share = np.histogram(draws[:, c].astype(np.float64), bins=edges[c])[0] / n
        bound = 6.0 * np.sqrt(p_all[c] * (1.0 - p_all[c]) / n) + 1e-5
        worst = max(worst, float((np.abs(share - p_all[c]) / bound).max()))
        assert (np.abs(share - p_all[c]) <= bound).all(), c
    print("largest |share - p| / bound:", worst)


# ---- 8: encode_dataset --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_encode_dataset_equals_the_encoder_batch_by_batch(jpeg_folder, dtype):
    torch.manual_seed(42)
    tl, vl, shape = V.data.get_dataset_loaders(jpeg_folder, batch_size=16, device=DEV, workers=1)
    e, _, _, _ = build(shape[1], dtype)
    e.eval()
    torch.manual_seed(7)                                                   # the train loader shuffles from the default RNG
    with torch.no_grad():
        want, sizes = [], []
        for loader in (tl, vl):
            for img in loader:
                mu, lv = e(img)
                want.append(torch.cat([mu, lv], 1))
                sizes.append(img.shape[0])
    want = torch.cat(want)
    assert sizes == [16, 16, 8, 5]                                         # ragged batches in both loaders
    e.train()
    before = {k: t.clone() for k, t in e.state_dict().items()}
    torch.manual_seed(7)
    got, n = V.encode_dataset(e, tl, vl)
    assert not e.training and n == 45
    assert got.dtype == torch.float32 and got.shape == (45, 200) and got.is_cuda
    assert torch.equal(got, want)
    after = e.state_dict()
    assert before.keys() == after.keys()
    for k in before:
        assert torch.equal(before[k], after[k]), k                        # BatchNorm buffers included
    with pytest.raises(RuntimeError):
        V.encode_dataset(e)
    pairs = data.DeviceLoader(tl.dataset, torch.arange(4), 2, degrade=data.Degrade(0.1))
    with pytest.raises(RuntimeError, match="clean batches"):
        V.encode_dataset(e, pairs)


# ---- 9: evaluate_generation ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_evaluate_generation_equals_the_loop_from_public_pieces(jpeg_folder, dtype):
    ds = data.ResidentImages.from_folder(jpeg_folder, device=DEV, workers=1)
    e, g, _, _ = build(64, dtype)
    allimgs = data.DeviceLoader(ds, torch.arange(len(ds)), 16)
    mulv, n = V.encode_dataset(e, allimgs)
    prior = V.LatentPrior.fit(mulv, 100)
    assert prior.n_fitted == n == 45
    vl = data.DeviceLoader(ds, torch.arange(30, 40), 4)                    # 4 + 4 + 2
    gen = torch.Generator().manual_seed(99)
    draws = []
    for b in (4, 4, 2):
        draws.append((torch.rand(b, 200, dtype=torch.float64, generator=gen).to(DEV),
                      torch.rand(b, 200, dtype=torch.float64, generator=gen).to(DEV),
                      torch.randn(b, 100, generator=gen).to(DEV)))
    calls = []

    def noise_fn(i, b):
        calls.append((i, b))
        return draws[i]
    got = V.evaluate_generation(g, vl, prior, noise_fn)
    assert calls == [(0, 4), (1, 4), (2, 2)] and not g.training
    assert got["samples"] == 10 and got["batches"] == 3
    g.eval()
    tot = 0.0
    with torch.no_grad():
        for (u, v, eps), real in zip(draws, vl):
            b = real.shape[0]
            z = prior.sample_z(b, g, u, v, eps)
            fake = g(z.view(b, -1)[:, :100].float().reshape(b, 100, 1, 1).contiguous())
            tot += b * float(ops.ssim(fake, real).item())
    want = tot / 10
    print("ssim", got["ssim"], "loop", want)
    assert abs(got["ssim"] - want) <= 1e-5
    # z ~ N(0, I): injected z against the same loop
    zs = [torch.randn(b, 100, generator=gen).to(DEV) for b in (4, 4, 2)]
    got0 = V.evaluate_generation(g, vl, None, lambda i, b: zs[i])
    tot = 0.0
    with torch.no_grad():
        for zz, real in zip(zs, vl):
            tot += real.shape[0] * float(ops.ssim(g(zz.view(-1, 100, 1, 1)), real).item())
    assert abs(got0["ssim"] - tot / 10) <= 1e-5
    # ... and from the device stream
    V.configure_seed(3)
    r = V.evaluate_generation(g, vl)
    assert math.isfinite(r["ssim"]) and -1.0 <= r["ssim"] <= 1.0
    assert r["samples"] == 10 and r["batches"] == 3
    assert int(ops.default_noise(prior.edges.device).state[1].item()) == 3  # one step of the stream per batch
    V.configure_seed(3)
    assert V.evaluate_generation(g, vl)["ssim"] == r["ssim"]
    rp = V.evaluate_generation(g, vl, prior)
    assert math.isfinite(rp["ssim"]) and -1.0 <= rp["ssim"] <= 1.0 and rp["samples"] == 10
    with pytest.raises(RuntimeError):
        V.evaluate_generation(g, [])


# ---- 10: uint8 pictures -------------------------------------------------------------------------------------------------
def torch_u8(x):
    return ((x + 1) / 2 * 255).clamp(0, 255).to(torch.uint8)


def test_to_u8_equals_torch_on_the_host_bitwise():
    B, C, H, W = 5, 3, 8, 20
    gen = torch.Generator().manual_seed(8)
    x = (torch.rand(B * C * H * W, generator=gen) * 2.2 - 1.1)
    k = torch.arange(256, dtype=torch.float32)
    special = torch.cat([torch.tensor([-1.0, 1.0, -1.0 - 1e-6, 1.0 + 1e-6, -1.5, 1.5, 0.0, -0.0]), k / 127.5 - 1,
                         torch.nextafter(k / 127.5 - 1, torch.tensor(-2.0)), torch.nextafter(k / 127.5 - 1, torch.tensor(2.0))])
    x[:special.numel()] = special
    x = x[torch.randperm(x.numel(), generator=gen)].view(B, C, H, W)
    want = torch_u8(x)
    assert want.min() == 0 and want.max() == 255 and len(want.unique()) == 256
    got = ops.to_u8(x.to(DEV))
    assert got.dtype == torch.uint8 and got.shape == (B, C, H, W)
    assert torch.equal(got.cpu(), want)
    for cols in (1, 2, 3, 5, 7):
        rows = (B + cols - 1) // cols
        pic = torch.zeros(rows * H, cols * W, C, dtype=torch.uint8)
        for i in range(B):
            r, c = divmod(i, cols)
            pic[r * H:(r + 1) * H, c * W:(c + 1) * W] = want[i].permute(1, 2, 0)
        got = ops.to_u8(x.to(DEV), cols)
        assert got.shape == pic.shape and torch.equal(got.cpu(), pic), cols


def test_sample_images_shapes_and_values():
    _, g, _, _ = build(64)
    V.configure_seed(1)
    pic = V.sample_images(g, n=64, grid_cols=8)
    assert pic.shape == (512, 512, 3) and pic.dtype == torch.uint8 and pic.is_cuda and not g.training
    assert V.sample_images(g, n=9).shape == (9, 3, 64, 64)
    fixed = torch.randn(64, 100, 1, 1, device=DEV)                         # vaegan_code.py:40
    imgs = V.sample_images(g, z=fixed)
    with torch.no_grad():
        want = torch_u8(g(fixed).cpu())
    assert torch.equal(imgs.cpu(), want)
    grid = V.sample_images(g, z=fixed, grid_cols=8).cpu()
    for i in (0, 7, 8, 63):
        r, c = divmod(i, 8)
        assert torch.equal(grid[r * 64:(r + 1) * 64, c * 64:(c + 1) * 64], want[i].permute(1, 2, 0))
    prior = V.LatentPrior.fit(torch.from_numpy(matrix(1000, 200, 2)).to(DEV) * 0.01, 100)
    assert V.sample_images(g, n=9, prior=prior, grid_cols=3).shape == (192, 192, 3)
    with pytest.raises(RuntimeError):
        V.sample_images(g, z=fixed, prior=prior)
    with pytest.raises(RuntimeError):
        V.sample_images(g, z=fixed[:, :50])


# ---- 11: state_dict -----------------------------------------------------------------------------------------------------
def test_state_dict_round_trips_through_torch_save(tmp_path):
    L = 6
    prior = V.LatentPrior.fit(torch.from_numpy(matrix(2000, 2 * L, 13)).to(DEV), L, n_bins=50)
    path = os.path.join(tmp_path, "prior.pth")
    torch.save(prior.state_dict(), path)
    sd = torch.load(path, weights_only=True)
    back = V.LatentPrior.from_state_dict(sd, DEV)
    assert (back.latent_dim, back.n_bins, back.n_fitted) == (L, 50, 2000)
    for name in ("edges", "counts", "cdf"):
        assert torch.equal(getattr(back, name), getattr(prior, name)) and getattr(back, name).is_cuda
    gen = torch.Generator().manual_seed(2)
    u = torch.rand(100, 2 * L, dtype=torch.float64, generator=gen).to(DEV)
    v = torch.rand(100, 2 * L, dtype=torch.float64, generator=gen).to(DEV)
    a, b = prior.sample(100, u, v), back.sample(100, u, v)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    other = V.LatentPrior.fit(torch.from_numpy(matrix(500, 2 * L, 14)).to(DEV), L)
    assert other.load_state_dict(sd) is other and other.n_bins == 50
    c = other.sample(100, u, v)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
