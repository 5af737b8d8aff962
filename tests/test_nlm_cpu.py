"""No GPU: the reference that the non-local-means baseline and the blind noise estimate are tested against
(tests/_nlm_ref.py) is itself checked -- the vectorised restatement against the definition written as loops, closed forms,
every pass-through rule, that the method denoises at all, the estimator against scipy and against known noise levels -- then
the exact-input table of the GPU test (exactness and blind spots, asserted on the reference alone), the exported symbols,
the host-side argument checks of the two C entry points and the validation of NLMeans / ``baseline=``."""
import ctypes
import os
import re
from importlib import import_module

import numpy as np
import pytest

import _nlm_ref as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
EINVAL, EALIGN = -1, -2


# ---- the restatement against the definition ----------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [0, 1, 2, 3])
@pytest.mark.parametrize("R", [1, 2, 4])
@pytest.mark.parametrize("C", [1, 3])
def test_restatement_equals_the_definition_written_as_loops(P, R, C):
    H, W = max(7, P + R + 1), max(9, P + R + 2)
    rng = np.random.default_rng(100 * P + 10 * R + C)
    x = rng.uniform(-1, 1, (2, C, H, W)).astype(np.float32)
    sigma = np.array([0.1, 0.3], dtype=np.float32)
    got = NR.nlm_ref(x, sigma, P, R, 0.8, 0.05)
    want = NR.nlm_naive(x, sigma, P, R, 0.8, 0.05)
    assert np.abs(got - want).max() < 1e-13


# ---- closed forms --------------------------------------------------------------------------------------------------------------
def test_closed_forms_constant_image_huge_h_and_tiny_h():
    rng = np.random.default_rng(3)
    const = np.full((1, 3, 9, 11), 0.375, dtype=np.float32)
    assert np.array_equal(NR.nlm_ref(const, np.array([0.1], np.float32), 2, 3, 0.8, 0.0), const.astype(np.float64))
    x = rng.uniform(-1, 1, (1, 2, 9, 11)).astype(np.float32)
    P, R = 1, 3
    # h -> infinity: every weight is 1, the output is the (2R+1)^2 box mean of the reflect-padded image
    got = NR.nlm_ref(x, None, P, R, 0.0, 1e18)
    xp = np.pad(x[0].astype(np.float64), ((0, 0), (R, R), (R, R)), mode="reflect")
    box = sum(xp[:, a:a + 9, b:b + 11] for a in range(2 * R + 1) for b in range(2 * R + 1)) / (2 * R + 1) ** 2
    assert np.abs(got[0] - box).max() < 1e-14
    # h tiny: only the centre (and exact twins, which random data does not have) survives
    assert np.array_equal(NR.nlm_ref(x, None, P, R, 0.0, 1e-6), x.astype(np.float64))


@pytest.mark.parametrize("sigma,hf,hc", [(np.nan, 0.8, 0.1), (np.inf, 0.8, 0.1), (-np.inf, 0.8, 0.1), (-1.0, 0.8, 0.1),
                                         (0.0, 0.8, 0.0), (-0.125, 0.8, 0.1), (3e38, 3e38, 0.0)])
def test_every_pass_through_rule(sigma, hf, hc):
    """h_b not finite or <= 0, or sigma_b not finite: the image is copied; its neighbour in the batch is filtered."""
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, (2, 1, 8, 8)).astype(np.float32)
    s = np.array([sigma, 0.25], dtype=np.float32)
    _, h, skip = NR.image_params(s, 0, hf, hc)
    assert skip and not NR.image_params(s, 1, 0.8, 0.1)[2]
    y = NR.nlm_ref(x, s, 1, 2, hf, hc) if np.isfinite(np.float32(hf) * 0.25 + hc) else None
    if y is not None:
        assert np.array_equal(y[0], x[0].astype(np.float64)) and not np.array_equal(y[1], x[1].astype(np.float64))
    with np.errstate(over="ignore"):
        assert np.array_equal(NR.nlm_naive(x[:1], s[:1], 1, 2, hf, hc)[0], x[0].astype(np.float64))


# ---- the method denoises ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synthetic():
    return NR.synthetic(64, 64)


@pytest.mark.parametrize("sigma", [0.05, 0.1, 0.2])
def test_nlm_gains_more_than_3_db_on_a_synthetic_image(synthetic, sigma):
    """A numpy prototype of this definition gave +5.7, +7.9 and +10.5 dB (P = 2, R = 7, h = 0.8 sigma)."""
    rng = np.random.default_rng(17)
    noisy = (synthetic + sigma * rng.standard_normal(synthetic.shape)).astype(np.float32)
    y = NR.nlm_ref(noisy, np.array([sigma], np.float32), 2, 7, 0.8, 0.0)
    gain = NR.psnr(y, synthetic) - NR.psnr(noisy, synthetic)
    print(f"sigma {sigma}: noisy {NR.psnr(noisy, synthetic):.2f} dB, nlm {NR.psnr(y, synthetic):.2f} dB, gain {gain:.2f} dB")
    assert gain > 3.0


# ---- the estimator -----------------------------------------------------------------------------------------------------------------
def test_mask_response_equals_scipy_convolve():
    from scipy.ndimage import convolve
    rng = np.random.default_rng(23)
    x = rng.standard_normal((2, 3, 13, 17))
    got = NR.mask_response(x)
    for b in range(2):
        for c in range(3):
            want = convolve(x[b, c], NR.MASK, mode="constant")[1:-1, 1:-1]
            assert np.abs(got[b, c] - want).max() < 1e-12
    s, S = NR.noise_sigma_ref(x.astype(np.float32))
    assert s.dtype == np.float32 and S.shape == (2,)
    assert s[0] == np.float32(np.abs(NR.mask_response(x.astype(np.float32)[0])).sum() * NR.noise_k(3, 13, 17))


@pytest.mark.parametrize("sigma", [0.05, 0.1, 0.2, 0.4])
def test_estimate_is_within_15_percent_of_the_noise_level(synthetic, sigma):
    """Prototype: 0.057, 0.106, 0.207, 0.400."""
    rng = np.random.default_rng(29)
    noisy = (synthetic + sigma * rng.standard_normal(synthetic.shape)).astype(np.float32)
    est = float(NR.noise_sigma_ref(noisy)[0][0])
    print(f"sigma {sigma}: estimate {est:.4f}")
    assert abs(est - sigma) <= 0.15 * sigma


# ---- the exact-input table: exactness and blind spots ---------------------------------------------------------------------------
def check_exact_cases(P, R):
    """Every assertion on the table's cases of one (P, R); -> the number of pixels ON the image border that have matches
    besides themselves, every one of which lies outside the image."""
    reflect_only = 0
    for C in NR.EXACT_C:
        for H, W in NR.exact_shapes(P, R):
            x, sigma = NR.exact_case(P, R, C, H, W)
            y, info = NR.nlm_exact(x, sigma, P, R)
            K = info["K"]
            counts = np.concatenate([c.ravel() for c in info["counts"] if c is not None])
            assert info["counts"][2] is None and np.array_equal(y[2], x[2])
            assert counts.min() == 1 and counts.max() == K and np.any((counts > 1) & (counts < K)), (P, R, C, H, W)
            assert info["soft_matches"][0] == 0 and info["soft_matches"][1] > 0, (P, R, C, H, W)
            assert not np.array_equal(y[:2], x[:2]), "the filter changes something (P = 0, sigma = 0: exact twins average to x)"
            for img in (0, 1):
                o = info["only_reflect"][img]
                edge = np.zeros_like(o)
                edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = True
                reflect_only += int((o & edge).sum())
            ref = NR.nlm_ref(x, sigma, P, R, NR.EXACT_HF, NR.EXACT_HC)
            assert np.abs(ref - y).max() <= 2.0 ** -22, "the restatement, whose weights are 1 or < 1e-55, agrees"
    return reflect_only


@pytest.mark.parametrize("P,R", NR.EXACT_PR)
def test_exact_table_is_exact_and_has_no_blind_spot(P, R):
    """What makes the bitwise GPU cases safe, asserted on the reference alone: nlm_exact itself asserts integer inputs in
    [-3, 3], integer patch sums, every weight exactly 1 or with a >= 128, no distance on the threshold, sums below 2^24.  Here:
    every case has pixels that match only themselves, pixels with the full count K and counts in between; image 1 (sigma > 0)
    has patches with 0 < d2 <= 2 sigma^2 that weigh exactly 1; the pass-through image comes back unchanged; the f64
    restatement agrees with the exact result; and (every (P, R) with P > 0 -- with P = 0 a pixel's reflected twin is the pixel
    itself or lies inside the image) there are pixels ON the image border with matches besides themselves, every one of which
    lies outside the image: a kernel that reflected wrongly could not pass the bitwise cases."""
    reflect_only = check_exact_cases(P, R)
    print(f"P {P} R {R}: border pixels matched only through reflection: {reflect_only}")
    assert reflect_only > 0 or P == 0


# ---- host checks -----------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported_with_the_abi_still_at_31():
    L = import_module(PKG + "._lib")
    lib = L.load()
    src = open(os.path.join(ROOT, "include", "vaegan_hip.h")).read()
    assert int(re.search(r"#define\s+VG_ABI_VERSION\s+(\d+)", src).group(1)) == L.ABI_VERSION == 31
    assert lib.vg_abi_version() == 31
    for name in ("vg_nlm_denoise", "vg_noise_sigma"):
        assert name in L.SIGNATURES and re.search(r"\b%s\s*\(" % name, src), name
        assert getattr(lib, name) is not None
    ops = import_module(PKG + ".ops")
    assert callable(ops.nlm_denoise) and callable(ops.noise_sigma)
    assert "nlm.hip" in open(os.path.join(ROOT, PKG, "csrc", "Makefile")).read()
    import vaegan_amd as V
    assert V.NLMeans is import_module(PKG + ".baselines").NLMeans and "NLMeans" in V.__all__


def test_c_abi_rejects_bad_arguments_of_both_entry_points_on_host():
    """Validation happens before any launch (pattern: test_host_cpu.test_c_abi_rejects_bad_arguments_on_host)."""
    lib = import_module(PKG + "._lib").load()
    x, y, s = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 26), ctypes.c_void_p(1 << 12)     # never dereferenced
    f = lib.vg_nlm_denoise
    ok = dict(x=x, y=y, B=3, C=3, H=32, W=40, P=2, R=7, sigma=s, stride=8, hf=0.8, hc=0.0, stream=None)

    def nl(**kw):
        return f(*dict(ok, **kw).values())

    inf, nan = float("inf"), float("nan")
    for kw in (dict(x=None), dict(y=None), dict(y=x), dict(y=ctypes.c_void_p((1 << 20) + 4 * 100)),
               dict(x=ctypes.c_void_p((1 << 26) + 4 * (3 * 3 * 32 * 40 - 1))),
               dict(B=0), dict(C=0), dict(H=0), dict(W=0), dict(B=-1), dict(C=5),
               dict(P=-1), dict(P=4), dict(R=0), dict(R=11),
               dict(H=9), dict(W=9), dict(H=9, W=9), dict(P=3, R=10, H=13), dict(P=0, R=1, H=1, W=64),
               dict(stride=0), dict(stride=-8),
               dict(hf=nan), dict(hf=inf), dict(hf=-0.5), dict(hc=nan), dict(hc=inf), dict(hc=-1e-3), dict(hf=0.0, hc=0.0),
               dict(B=65536, C=1, H=16, W=16), dict(B=1, C=1, H=16 * 65536, W=16), dict(B=8, C=4, H=8192, W=8192),
               dict(B=65535, C=1, H=16, W=16, stride=1 << 16)):
        assert nl(**kw) == EINVAL, kw
    assert nl(x=ctypes.c_void_p((1 << 20) + 2)) == EALIGN and nl(sigma=ctypes.c_void_p((1 << 12) + 1)) == EALIGN

    g = lib.vg_noise_sigma
    ok = dict(x=x, B=3, C=3, H=32, W=40, sigma=s, stride=1, stream=None)

    def ns(**kw):
        return g(*dict(ok, **kw).values())

    for kw in (dict(x=None), dict(sigma=None), dict(B=0), dict(C=0), dict(H=2), dict(W=2), dict(H=0), dict(stride=0),
               dict(stride=-1), dict(C=1 << 20, H=1 << 12), dict(B=1 << 20, stride=1 << 12)):
        assert ns(**kw) == EINVAL, kw
    assert ns(x=ctypes.c_void_p((1 << 20) + 2)) == EALIGN and ns(sigma=ctypes.c_void_p((1 << 12) + 3)) == EALIGN


def test_nlmeans_and_baseline_keyword_validation():
    import vaegan_amd as V
    B = import_module(PKG + ".baselines")
    n = V.NLMeans()
    assert (n.patch_radius, n.search_radius, n.h_factor, n.sigma, n.needs_rects) == (2, 7, B.DEFAULT_H_FACTOR, "oracle", True)
    assert not V.NLMeans(sigma="estimate").needs_rects and V.NLMeans(sigma=0.1).sigma == 0.1
    for kw in (dict(patch_radius=-1), dict(patch_radius=4), dict(patch_radius=1.0), dict(patch_radius=True),
               dict(search_radius=0), dict(search_radius=11), dict(search_radius="7"),
               dict(h_factor=0.0), dict(h_factor=-1.0), dict(h_factor=float("nan")), dict(h_factor=float("inf")), dict(h_factor="1"),
               dict(sigma="blind"), dict(sigma=0.0), dict(sigma=-0.1), dict(sigma=float("nan")), dict(sigma=None), dict(sigma=True)):
        with pytest.raises(ValueError):
            V.NLMeans(**kw)
    import torch
    with pytest.raises(RuntimeError, match="cuda"):
        n(torch.zeros(1, 3, 16, 16))
    assert B.make_baseline("t", None) is None and B.make_baseline("t", n) is n
    assert B.make_baseline("t", "nlm").sigma == "oracle" and B.make_baseline("t", "nlm", allow_oracle=False).sigma == "estimate"
    assert B.make_baseline("t", dict(sigma=0.2, search_radius=5)).search_radius == 5
    for bad in ("bm3d", 7, dict(radius=3), dict(sigma="blind")):
        with pytest.raises(ValueError):
            B.make_baseline("t", bad)
    for bad in (n, dict(sigma="oracle"), dict()):
        with pytest.raises(ValueError, match="estimate"):
            B.make_baseline("t", bad, allow_oracle=False)
    # the passes validate the keyword before they touch a network or a loader
    for fn in (V.paired_test_epoch, V.tiled_test_epoch):
        with pytest.raises(ValueError, match="baseline"):
            fn(None, None, [], baseline="bm3d")
    with pytest.raises(ValueError, match="estimate"):
        V.tiled_test_epoch(None, None, [], baseline=V.NLMeans())
