"""GPU: the non-local-means baseline and the blind noise estimate from the kernels up -- vg_nlm_denoise bit for bit on the
exact-input table of tests/_nlm_ref.py (whose exactness and blind spots tests/test_nlm_cpu.py asserts) and within twice the
counted first-order bound on random inputs, repeatability, graph replay and image independence; vg_noise_sigma bit for bit
on integer images and within its counted bound on random ones; NLMeans and ``baseline=`` of the two test passes."""
import importlib
import math
import os

import numpy as np
import pytest
import torch

import _nlm_ref as NR

import vaegan_amd as V
from test_gpu_data import jpeg_folder  # noqa: F401  (fixture: 45 generated 64 x 64 JPEGs)

pytestmark = pytest.mark.gpu
DEV = "cuda"
torch.set_num_threads(min(16, os.cpu_count() or 1))

PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
ops = importlib.import_module(PKG + ".ops")
data = importlib.import_module(PKG + ".data")
U = 2.0 ** -24
SENTINEL = 1234.5
PRC = [(P, R, C) for P, R in NR.EXACT_PR for C in NR.EXACT_C]
PRC_IDS = [f"P{P}R{R}C{C}" for P, R, C in PRC]


def run_nlm(x, sigma, P, R, hf, hc, misalign=0):
    """x numpy f32 [B,C,H,W], sigma numpy f32 [B] -> y numpy f32.  x's base sits ``misalign`` floats past a 256-byte boundary;
    sigma is read through a stride of 8 from column 1 of a [B, 8] tensor; the destination is NaN-filled and lies between two
    sentinel rows that must survive."""
    B, C, H, W = x.shape
    n = x.size
    xbuf = torch.empty(n + misalign, dtype=torch.float32, device=DEV)
    xd = xbuf[misalign:].view(B, C, H, W)
    xd.copy_(torch.from_numpy(x))
    assert xd.data_ptr() % 16 == (4 * misalign) % 16
    rects = torch.full((B, 8), float("nan"), dtype=torch.float32, device=DEV)
    rects[:, 1] = torch.from_numpy(sigma)
    ybuf = torch.full((n + 2 * W,), float("nan"), dtype=torch.float32, device=DEV)
    ybuf[:W] = SENTINEL
    ybuf[W + n:] = SENTINEL
    yd = ybuf[W:W + n].view(B, C, H, W)
    out = ops.nlm_denoise(xd, rects[:, 1], patch_radius=P, search_radius=R, h_factor=hf, h_const=hc, out=yd)
    assert out is yd
    host = ybuf.cpu().numpy()
    assert np.all(host[:W] == SENTINEL) and np.all(host[W + n:] == SENTINEL), "the sentinel rows survive"
    assert np.array_equal(xd.cpu().numpy(), x), "the input is not written"
    return host[W:W + n].reshape(B, C, H, W)


# ======================================================================================================================
# vg_nlm_denoise
# ======================================================================================================================
@pytest.mark.parametrize("P,R,C", PRC, ids=PRC_IDS)
def test_nlm_is_bit_exact_on_the_exact_input_table(P, R, C):
    for k, (H, W) in enumerate(NR.exact_shapes(P, R)):
        x, sigma = NR.exact_case(P, R, C, H, W)
        want, _ = NR.nlm_exact(x, sigma, P, R)
        got = run_nlm(x, sigma, P, R, NR.EXACT_HF, NR.EXACT_HC, misalign=k % 2)    # every other shape 4 bytes off the 16-byte grid
        assert not np.isnan(got).any(), (H, W)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (H, W, int((got != want).sum()))


def random_case(P, R, C, H, W):
    """Three images in [-1, 1]: smooth structure plus noise of the level the filter is then told (0.08 and 0.25), and a
    pass-through image (sigma = NaN)."""
    rng = np.random.default_rng(7 * P + 11 * R + 13 * C + H * 17 + W)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([0.6 * np.sin(0.7 * xx + 0.3 * c) * np.cos(0.45 * yy - 0.2 * c) for c in range(C)])
    sig = np.array([0.08, 0.25, np.nan], dtype=np.float32)
    x = np.stack([base + 0.08 * rng.standard_normal(base.shape), base + 0.25 * rng.standard_normal(base.shape),
                  rng.uniform(-1, 1, base.shape)]).astype(np.float32)
    return x, sig


@pytest.mark.parametrize("P,R,C", PRC, ids=PRC_IDS)
def test_nlm_random_inputs_within_twice_the_counted_bound(P, R, C):
    """|y - y_ref| <= 2 x bound(p) element-wise (tests/_nlm_ref.py: the first-order bound counted from the kernel's operation
    sequence; the factor 2 covers the second-order terms).  h = 0.8 sigma + 0.02.  Measured on an MI355X (DESIGN.md section
    4.4r): the largest ratio |y - y_ref| / bound is 0.24 (P = 0, R = 1, C = 4), 0.02 .. 0.06 for the wider windows."""
    worst = 0.0
    for k, (H, W) in enumerate(NR.exact_shapes(P, R)):
        x, sigma = random_case(P, R, C, H, W)
        want, bound = NR.nlm_ref(x, sigma, P, R, 0.8, 0.02, want_bound=True)
        got = run_nlm(x, sigma, P, R, 0.8, 0.02, misalign=(k + 1) % 2)
        assert np.array_equal(got[2].view(np.uint32), x[2].view(np.uint32)), "the pass-through image is copied bit for bit"
        err = np.abs(got[:2].astype(np.float64) - want[:2])
        ratio = float((err / bound[:2]).max())
        worst = max(worst, ratio)
        print(f"P {P} R {R} C {C} {H}x{W}: max err {err.max():.3e}, max bound {bound[:2].max():.3e}, max err/bound {ratio:.4f}")
        assert np.all(err <= 2.0 * bound[:2]), (H, W, ratio)
    print(f"P {P} R {R} C {C}: largest err/bound {worst:.4f}")


def test_nlm_is_repeatable_replays_from_a_graph_and_keeps_images_apart():
    P, R, C, H, W = 2, 5, 3, 19, 37
    x, sigma = random_case(P, R, C, H, W)
    sigma[2] = 0.15
    xd, sd = torch.from_numpy(x).to(DEV), torch.from_numpy(sigma).to(DEV)
    kw = dict(patch_radius=P, search_radius=R, h_factor=0.8, h_const=0.02)
    y1 = ops.nlm_denoise(xd, sd, **kw)
    y2 = ops.nlm_denoise(xd, sd, **kw)
    assert torch.equal(y1, y2), "two runs agree bit for bit"
    yg = torch.full_like(y1, float("nan"))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):                                       # one stream, no parallel branches
            ops.nlm_denoise(xd, sd, out=yg, **kw)
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(yg, y1), "a graph replay agrees with the eager launch bit for bit"
    # image independence: another image 1 leaves image 0's bits alone; a NaN image leaves its neighbours finite
    x2 = xd.clone()
    x2[1] = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, (C, H, W)).astype(np.float32)).to(DEV)
    y3 = ops.nlm_denoise(x2, sd, **kw)
    assert torch.equal(y3[0], y1[0]) and torch.equal(y3[2], y1[2]) and not torch.equal(y3[1], y1[1])
    x2[1] = float("nan")
    y4 = ops.nlm_denoise(x2, sd, **kw)
    assert torch.equal(y4[0], y1[0]) and torch.equal(y4[2], y1[2]) and bool(torch.isnan(y4[1]).all())
    # the sigma forms: None is 0 (h = h_const), a float is materialised, a [B] tensor and a strided view are read in place
    wide = torch.zeros(3, 8, device=DEV)
    wide[:, 1] = 0.15
    a = ops.nlm_denoise(xd, 0.15, **kw)
    assert torch.equal(a, ops.nlm_denoise(xd, wide[:, 1], **kw)) and torch.equal(a, ops.nlm_denoise(xd, torch.full((3,), 0.15, device=DEV), **kw))
    assert torch.equal(ops.nlm_denoise(xd, None, **kw), ops.nlm_denoise(xd, 0.0, **kw))
    for bad in (dict(sigma=torch.zeros(2, device=DEV)), dict(sigma=torch.zeros(3)), dict(sigma=torch.zeros(3, 1, device=DEV)),
                dict(sigma=torch.zeros(3, dtype=torch.float64, device=DEV)), dict(out=xd), dict(out=torch.empty(3, C, H, W + 1, device=DEV))):
        with pytest.raises(RuntimeError):
            ops.nlm_denoise(xd, **{"sigma": sd, **bad}, **kw)
    with pytest.raises(RuntimeError, match="VG_EINVAL"):
        ops.nlm_denoise(xd[:, :, :7].contiguous(), sd, **kw)                      # 7 rows < P + R + 1


# ======================================================================================================================
# vg_noise_sigma
# ======================================================================================================================
@pytest.mark.parametrize("C,H,W", [(1, 3, 3), (3, 5, 7), (4, 17, 70), (3, 64, 64), (2, 3, 130)])
def test_noise_sigma_is_bit_exact_on_integer_images_and_within_its_bound_on_random_ones(C, H, W):
    """Integer images: the mask responses and their sum are exact in f64, so the result is (float)(S * k) bit for bit.
    Random images: the device sum differs from the restatement's by the order of n f64 additions and the nine-term response:
    |got - S k| <= (2^-24 + (n + 16) 2^-53) S k.  B = 3, the output strided through a [B, 4] tensor whose other columns survive."""
    rng = np.random.default_rng(C * 100 + H * 10 + W)
    n = C * (H - 2) * (W - 2)
    for kind in ("int", "random"):
        x = (rng.integers(-9, 10, (3, C, H, W)) if kind == "int" else rng.standard_normal((3, C, H, W))).astype(np.float32)
        want, S = NR.noise_sigma_ref(x)
        xd = torch.from_numpy(x).to(DEV)
        wide = torch.full((3, 4), SENTINEL, device=DEV)
        out = ops.noise_sigma(xd, out=wide[:, 1])
        assert out.data_ptr() == wide[:, 1].data_ptr()
        host = wide.cpu().numpy()
        assert np.all(host[:, [0, 2, 3]] == SENTINEL)
        got = host[:, 1]
        if kind == "int":
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)
        else:
            exact = S * NR.noise_k(C, H, W)
            assert np.all(np.abs(got.astype(np.float64) - exact) <= (2.0 ** -24 + (n + 16) * 2.0 ** -53) * exact), (got, exact)
        again = ops.noise_sigma(xd)
        assert again.shape == (3,) and np.array_equal(again.cpu().numpy().view(np.uint32), got.view(np.uint32)), "repeatable"
    with pytest.raises(RuntimeError):
        ops.noise_sigma(xd, out=torch.empty(2, device=DEV))
    with pytest.raises(RuntimeError):
        ops.noise_sigma(xd.double())
    if H == 3 and W == 3:
        with pytest.raises(RuntimeError, match="VG_EINVAL"):
            ops.noise_sigma(xd[:, :, :2].contiguous())


# ======================================================================================================================
# NLMeans and baseline= of the two test passes
# ======================================================================================================================
NLM_KEYS = {"recon_loss_nlm", "ssim_nlm", "psnr_nlm"}
REGION_NLM = {k + "_nlm" for k in ("mse_hole", "mse_valid", "psnr_hole", "psnr_valid", "hole_fraction")}


@pytest.fixture(scope="module")
def nets():
    S = 64
    V.configure_seed(42)
    e, g = V.Encoder([3, S, S], 100), V.Generator(nz=100, img_size=S)
    g.apply(V.weights_init)
    return e.to(DEV), g.to(DEV)


def test_nlmeans_call_forms(jpeg_folder):  # noqa: F811
    ds = data.ResidentImages.from_folder(jpeg_folder, device=DEV, workers=1)
    loader = data.DeviceLoader(ds, torch.arange(0, 6), 6, shuffle=False, degrade=data.Degrade(0.2, rect=False))
    loader.want_rects(True)
    noisy, clean = next(iter(loader))
    rects = loader.last_rects.clone()
    loader.want_rects(False)
    oracle = V.NLMeans()(noisy, rects=rects)
    assert torch.equal(oracle, ops.nlm_denoise(noisy.contiguous(), rects[:, 1], patch_radius=2, search_radius=7, h_factor=0.8))
    est = V.NLMeans(sigma="estimate")(noisy)
    sig = ops.noise_sigma(noisy.contiguous())
    assert torch.equal(est, ops.nlm_denoise(noisy.contiguous(), sig, patch_radius=2, search_radius=7, h_factor=0.8))
    fixed = V.NLMeans(sigma=0.1, patch_radius=1, search_radius=5, h_factor=0.6)(noisy)
    assert torch.equal(fixed, ops.nlm_denoise(noisy.contiguous(), 0.1, patch_radius=1, search_radius=5, h_factor=0.6))
    print("sigma drawn", rects[:, 1].tolist(), "estimated", sig.tolist())
    with pytest.raises(RuntimeError, match="rects"):
        V.NLMeans()(noisy)
    with pytest.raises(RuntimeError, match="rects"):
        V.NLMeans()(noisy, rects=rects[:, :4])
    with pytest.raises(RuntimeError):
        V.NLMeans(sigma=0.1)(noisy.double())


def test_paired_test_epoch_baseline_keys_equal_the_loop_built_from_public_pieces(nets, jpeg_folder):  # noqa: F811
    e, g = nets
    ds = data.ResidentImages.from_folder(jpeg_folder, device=DEV, workers=1)
    loader = data.DeviceLoader(ds, torch.arange(40, 45), 2, shuffle=False, degrade=data.Degrade(0.25))
    eps = [torch.randn(b, 100, generator=torch.Generator().manual_seed(60 + i)) for i, b in enumerate((2, 2, 1))]
    noise_fn = lambda i, noisy: eps[i].to(DEV)                                  # noqa: E731
    torch.manual_seed(5)
    base = V.paired_test_epoch(e, g, loader, noise_fn=noise_fn)
    torch.manual_seed(5)
    none = V.paired_test_epoch(e, g, loader, noise_fn=noise_fn, baseline=None)
    assert none == base and list(none) == list(base), "baseline=None: today's keys and numbers, bit for bit"
    torch.manual_seed(5)
    got = V.paired_test_epoch(e, g, loader, noise_fn=noise_fn, baseline="nlm")
    assert set(got) == set(base) | NLM_KEYS and all(got[k] == base[k] for k in base)
    assert loader._rects is False and loader.last_rects is None, "want_rects is withdrawn"
    loader.want_rects(True)
    torch.manual_seed(5)
    V.paired_test_epoch(e, g, loader, noise_fn=noise_fn, baseline=V.NLMeans())
    assert loader._rects is True, "... and left on where it was on"
    loader.want_rects(False)
    torch.manual_seed(5)
    both = V.paired_test_epoch(e, g, loader, noise_fn=noise_fn, baseline=dict(sigma="oracle"), regions=True, ms_ssim=True)
    assert NLM_KEYS | REGION_NLM | {"ms_ssim_nlm"} <= set(both) and all(both[k] == got[k] for k in NLM_KEYS)
    # the loop from public pieces
    loader.want_rects(True)
    acc_ssim = acc_mse = acc_ms = 0.0
    stats = torch.zeros(4, dtype=torch.float64, device=DEV)
    seen = 0
    torch.manual_seed(5)
    for noisy, clean in loader:
        b = clean.shape[0]
        noisy, clean = noisy.contiguous(), clean.contiguous()
        f = ops.nlm_denoise(noisy, loader.last_rects[:, 1], patch_radius=2, search_radius=7, h_factor=0.8)
        slot = torch.empty(1, device=DEV)
        ops.mse_forward_backward(f, clean, 1.0, slot, False)
        acc_mse += b * float(slot)
        acc_ssim += b * float(ops.ssim(f, clean))
        acc_ms += b * float(ops.ms_ssim(f, clean))
        ops.region_mse_forward_backward(f, clean, loader.last_rects, 1.0, 1.0, stats=stats)
        seen += b
    loader.want_rects(False)
    s_hole, s_valid, n_hole, n_valid = stats.tolist()
    print("nlm", {k: both[k] for k in sorted(NLM_KEYS | REGION_NLM)}, "noisy", base["psnr_noisy"], base["ssim_noisy"])
    # the pass accumulates b * value in f32 on the device, this loop in f64 on the host: a few f32 roundings
    assert both["recon_loss_nlm"] == pytest.approx(acc_mse / seen, rel=8 * U)
    assert both["ssim_nlm"] == pytest.approx(acc_ssim / seen, rel=8 * U)
    assert both["ms_ssim_nlm"] == pytest.approx(acc_ms / seen, rel=8 * U)
    assert both["psnr_nlm"] == pytest.approx(10 * math.log10(4.0 / (acc_mse / seen)), abs=1e-4)
    assert both["mse_hole_nlm"] == s_hole / n_hole and both["mse_valid_nlm"] == s_valid / n_valid
    assert both["hole_fraction_nlm"] == n_hole / (n_hole + n_valid) == both["hole_fraction"]
    assert both["psnr_hole_nlm"] == 10.0 * math.log10(1.0 / (s_hole / n_hole / 4.0))
    assert both["psnr_valid_nlm"] == 10.0 * math.log10(1.0 / (s_valid / n_valid / 4.0))
    # "estimate" and a number run on a loader without rectangles; "oracle" is refused there
    torch.manual_seed(5)
    pairs = [(n.clone(), c.clone()) for n, c in loader]
    torch.manual_seed(5)
    est = V.paired_test_epoch(e, g, pairs, noise_fn=noise_fn, baseline=dict(sigma="estimate"))
    torch.manual_seed(5)
    num = V.paired_test_epoch(e, g, pairs, noise_fn=noise_fn, baseline=V.NLMeans(sigma=0.1))
    assert NLM_KEYS <= set(est) and NLM_KEYS <= set(num) and est["psnr_nlm"] != num["psnr_nlm"]
    with pytest.raises(RuntimeError, match="want_rects"):
        V.paired_test_epoch(e, g, pairs, noise_fn=noise_fn, baseline="nlm")
    with pytest.raises(ValueError, match="baseline"):
        V.paired_test_epoch(e, g, loader, baseline="bm3d")


def test_nlm_beats_the_noisy_input_on_the_generated_set(nets, jpeg_folder):  # noqa: F811
    e, g = nets
    ds = data.ResidentImages.from_folder(jpeg_folder, device=DEV, workers=1)
    flat = data.DeviceLoader(ds, torch.arange(0, 45), 15, shuffle=False, degrade=data.Degrade(0.2, rect=False))
    out = V.paired_test_epoch(e, g, flat, baseline="nlm")
    blind = V.paired_test_epoch(e, g, flat, baseline=dict(sigma="estimate"))
    print("psnr noisy", out["psnr_noisy"], "nlm oracle", out["psnr_nlm"], "nlm estimate", blind["psnr_nlm"],
          "ssim noisy", out["ssim_noisy"], "nlm", out["ssim_nlm"])
    assert out["psnr_nlm"] > out["psnr_noisy"] and out["samples"] == 45
    assert flat._rects is False


def test_tiled_test_epoch_baseline_is_nlm_of_the_whole_image(nets):
    e, g = nets
    rng = np.random.default_rng(3)
    clean = torch.from_numpy(NR.synthetic(96, 80).astype(np.float32)).to(DEV)
    noisy = (clean + 0.1 * torch.from_numpy(rng.standard_normal((1, 3, 96, 80)).astype(np.float32)).to(DEV)).clamp(-1, 1)
    base = V.tiled_test_epoch(e, g, [(noisy, clean)], stride=48, sample=False)
    out = V.tiled_test_epoch(e, g, [(noisy, clean)], stride=48, sample=False, baseline=dict(sigma=0.1), ms_ssim=True)
    assert set(out) == set(base) | NLM_KEYS | {"ms_ssim", "ms_ssim_noisy", "ms_ssim_nlm"} and all(out[k] == base[k] for k in base)
    f = ops.nlm_denoise(noisy, 0.1, patch_radius=2, search_radius=7, h_factor=0.8)
    slot = torch.empty(1, device=DEV)
    ops.mse_forward_backward(f, clean, 1.0, slot, False)
    assert out["recon_loss_nlm"] == pytest.approx(float(slot), rel=4 * U)
    assert out["ssim_nlm"] == pytest.approx(float(ops.ssim(f, clean)), rel=4 * U)
    assert out["ms_ssim_nlm"] == pytest.approx(float(ops.ms_ssim(f, clean)), rel=4 * U)
    assert out["psnr_nlm"] > out["psnr_noisy"]
    blind = V.tiled_test_epoch(e, g, [(noisy, clean)], stride=48, sample=False, baseline="nlm")
    fe = ops.nlm_denoise(noisy, ops.noise_sigma(noisy), patch_radius=2, search_radius=7, h_factor=0.8)
    ops.mse_forward_backward(fe, clean, 1.0, slot, False)
    assert blind["recon_loss_nlm"] == pytest.approx(float(slot), rel=4 * U)
    with pytest.raises(ValueError, match="estimate"):
        V.tiled_test_epoch(e, g, [(noisy, clean)], baseline=V.NLMeans())
