"""CPU: the noise models of the degraded pairs and the median baseline, host side -- the restatement
(tests/_noise_models_ref.py) against what it restates, the argument checks of the new C entry points, the validation of the
Python surface.  No GPU: the impulses are checked on host Philox words alone."""
import ctypes
import math
import os
import re
from importlib import import_module

import numpy as np
import pytest
import torch

import _noise_models_ref as R
import _philox_ref as P

PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
data = import_module(PKG + ".data")
baselines = import_module(PKG + ".baselines")
F = np.float32


# ---- the restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rect", [True, False])
def test_gaussian_without_impulses_is_the_old_expression_bitwise(rect):
    from test_gpu_degrade import add_noise_ref
    rng = np.random.default_rng(7)
    C, H, W = 3, 20, 24
    for trial in range(8):
        clean = (rng.integers(0, 256, (C, H, W)).astype(F) / F(255.0) - F(0.5)) / F(0.5)
        n = rng.standard_normal((C, H, W)).astype(F) * F(1.7)
        fill = (rng.integers(0, 1 << 24, (C, H, W)).astype(F) * F(2.0 ** -24))
        s = float(F(rng.integers(0, 1 << 24)) * F(2.0 ** -24))
        rh, rw, x, y = 5, 7, 3 + trial, 2 + trial
        want = add_noise_ref(torch.from_numpy(clean), torch.from_numpy(n), torch.from_numpy(fill), s, 0.3, rect, rh, rw, x, y)
        got = R.degrade_ref(clean, n, s, 0.3, R.GAUSSIAN, True, fill, (rh, rw, x, y) if rect else None)
        assert got.dtype == F and np.array_equal(got.view(np.uint32), want.numpy().view(np.uint32))
        assert (np.abs(got) == 1.0).any()                                 # the clamp took part


@pytest.mark.parametrize("kind,power", [(R.SPECKLE, 2), (R.SHOT, 1)])
def test_variance_of_the_noise_follows_the_intensity(kind, power):
    """Per intensity bin, Var(t - base) = level^2 * g^power with level = s * noise_max_std (the standard deviation at white).
    M normals per bin: the sample variance of M normal values has relative standard deviation sqrt(2 / (M - 1)); the bound is
    5 of them (the f32 rounding of t - base, below 1e-5 of the noise, is far inside)."""
    M, s, nms = 20000, 0.5, 0.1                                          # level 0.05: 6.8 sigma = 0.34 < 0.4, nothing is clamped
    level = float(F(s) * F(nms))
    rng = np.random.default_rng(11 + kind)
    bound = 5 * math.sqrt(2.0 / (M - 1))
    ratios = []
    for g in (0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8):
        base = np.full((1, 1, M), F(2 * g - 1), F)
        n = rng.standard_normal((1, 1, M)).astype(F)
        t = R.degrade_ref(base, n, s, nms, kind, True)
        assert float(np.abs(t).max()) < 1.0
        g32 = float((base[0, 0, 0] + F(1.0)) / F(2.0))
        var = float(np.var((t - base).astype(np.float64)))
        ratios.append(var / (level ** 2 * g32 ** power))
    print("variance / (level^2 g^%d) per bin:" % power, [round(r, 4) for r in ratios], "bound 1 +-", round(bound, 4))
    assert all(abs(r - 1.0) <= bound for r in ratios)
    # and normalize=False maps the same intensities: g is the value itself
    base = np.full((1, 1, M), F(0.5), F)
    t = R.degrade_ref(base, rng.standard_normal((1, 1, M)).astype(F), s, nms, kind, False)
    assert abs(float(np.var((t - base).astype(np.float64))) / (level ** 2 * 0.5 ** power) - 1.0) <= bound


@pytest.mark.parametrize("kind", [R.SPECKLE, R.SHOT])
def test_negative_intensity_of_a_fill_is_clamped_to_zero(kind):
    """normalize=False: lo = 0, span = 1, and a rectangle fill 2u - 1 with u < 0.5 is negative.  g = max(., 0) = 0, so f = 0
    (no root of a negative number) and the pixel keeps its fill whatever the normal."""
    C, H, W = 1, 4, 4
    clean = np.full((C, H, W), F(0.25), F)
    fill = np.full((C, H, W), F(0.125), F)                                # 2u - 1 = -0.75
    n = np.full((C, H, W), F(3.0), F)
    t = R.degrade_ref(clean, n, 0.9, 0.5, kind, False, fill, (2, 2, 1, 1))
    assert np.isfinite(t).all()
    assert (t[0, 1:3, 1:3] == F(-0.75)).all()
    f = 0.25 if kind == R.SPECKLE else 0.5
    outside = np.ones((H, W), bool)
    outside[1:3, 1:3] = False
    want = F(0.25) + ((F(3.0) * F(0.9)) * F(0.5)) * F(f)
    assert (t[0][outside] == min(want, F(1.0))).all()


# ---- impulses on host Philox words ---------------------------------------------------------------------------------------------
SEED, C, H, W = 20240607, 3, 32, 32


def test_impulse_counts_on_host_philox_words():
    n = C * H * W
    worst_hit = worst_salt = 0.0
    for pos in range(16):
        hit, salt, p_b = R.impulse_masks(SEED, pos, n, 0.3, 0.5)
        p = float(p_b)
        assert 0.0 <= p < 0.3
        hits, salts = int(hit.sum()), int(salt.sum())
        sd = math.sqrt(n * p * (1 - p))
        z_hit = abs(hits - n * p) / sd
        z_salt = abs(salts - hits / 2) / math.sqrt(hits * 0.25)
        worst_hit, worst_salt = max(worst_hit, z_hit), max(worst_salt, z_salt)
        assert z_hit <= 4.0 and z_salt <= 4.0, (pos, hits, n * p, salts)
        assert not (salt & ~hit).any()
    print(f"worst |z| over 16 images: hits {worst_hit:.2f}, salt {worst_salt:.2f}")


def test_impulse_extremes_on_host_philox_words():
    n = C * H * W
    for pos in (0, 5, 15):
        hit, salt, _ = R.impulse_masks(SEED, pos, n, 0.3, 0.0)
        assert hit.any() and not salt.any()                                # pepper only
        hit1, salt1, _ = R.impulse_masks(SEED, pos, n, 0.3, 1.0)
        assert np.array_equal(hit, hit1) and np.array_equal(salt1, hit1)   # salt only, the same elements
        hit0, salt0, p0 = R.impulse_masks(SEED, pos, n, 0.0, 0.5)
        assert p0 == 0 and not hit0.any() and not salt0.any()
    # in the restatement: hit elements are exactly lo or 1, the others untouched
    hit, salt, _ = R.impulse_masks(SEED, 3, n, 0.3, 0.5)
    iu = P.u01(P.words(SEED, 3, R.DRAW_IMPULSE, n)).reshape(C, H, W)
    su = P.u01(P.words(SEED, 3, R.DRAW_SALT, n)).reshape(C, H, W)
    clean = np.full((C, H, W), F(0.25), F)
    zero = np.zeros((C, H, W), F)
    for normalize, lo in ((True, -1.0), (False, 0.0)):
        t = R.degrade_ref(clean, zero, R.severity(SEED, 3), 0.2, R.SHOT, normalize, impulse_u=iu, salt_u=su, impulse_max_p=0.3)
        h, sa = hit.reshape(C, H, W), salt.reshape(C, H, W)
        assert (t[sa] == 1.0).all() and (t[h & ~sa] == lo).all() and (t[~h] == 0.25).all()


# ---- the median restatement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,shape", [(1, (2, 2)), (1, (3, 7)), (1, (10, 7)), (1, (16, 16)),
                                     (2, (3, 3)), (2, (3, 7)), (2, (10, 7)), (2, (16, 16))])
def test_median_restatement_equals_scipy(r, shape):
    import scipy.ndimage as ndi
    rng = np.random.default_rng(r * 100 + shape[0] * 10 + shape[1])
    x = rng.standard_normal((2, 3) + shape).astype(F)
    got = R.median_ref(x, r)
    assert got.dtype == F and got.shape == x.shape
    for b in range(2):
        for c in range(3):
            assert np.array_equal(got[b, c], ndi.median_filter(x[b, c], size=2 * r + 1, mode="mirror"))


# ---- the C entry points: every host argument check ---------------------------------------------------------------------------
BAD_MODELS = [(-1, 0.0, 0.5), (3, 0.0, 0.5), (0, -0.01, 0.5), (1, 1.01, 0.5), (2, math.nan, 0.5), (0, math.inf, 0.5),
              (0, 0.1, -0.01), (1, 0.1, 1.01), (2, 0.1, math.nan), (2, 0.1, -math.inf)]


def test_c_abi_of_the_new_entry_points_rejects_bad_arguments_on_host():
    L = import_module(PKG + "._lib")
    lib = L.load()
    buf = ctypes.c_void_p(256)                                           # never dereferenced: validation comes first
    b64 = data.degrade_bounds(64, 64)
    head = (buf, 10, buf, 4, 3, 64, 64, 1, 0, 0.25, 1, 1)
    tail = (buf, buf, None, 0, 0)
    for kind, p, sr in BAD_MODELS:
        assert lib.vg_gather_degrade_u8_ex(*head, *b64, *tail, kind, p, sr, None) == -1, (kind, p, sr)
        assert lib.vg_degrade_params_ex(1, 0, 4, 0.25, 1, 64, 64, *b64, buf, kind, p, sr, None) == -1, (kind, p, sr)
    ok = (2, 0.3, 0.5)
    # everything the old entry points refuse, with a valid model
    assert lib.vg_gather_degrade_u8_ex(None, 10, buf, 4, 3, 64, 64, 1, 0, 0.25, 1, 1, *b64, *tail, *ok, None) == -1
    assert lib.vg_gather_degrade_u8_ex(buf, 10, None, 4, 3, 64, 64, 1, 0, 0.25, 1, 1, *b64, *tail, *ok, None) == -1
    assert lib.vg_gather_degrade_u8_ex(*head, *b64, None, buf, None, 0, 0, *ok, None) == -1             # clean NULL
    assert lib.vg_gather_degrade_u8_ex(*head, *b64, buf, None, None, 0, 0, *ok, None) == -1             # noisy NULL
    assert lib.vg_gather_degrade_u8_ex(buf, 10, buf, 0, 3, 64, 64, 1, 0, 0.25, 1, 1, *b64, *tail, *ok, None) == -1    # B == 0
    assert lib.vg_gather_degrade_u8_ex(buf, 10, buf, 4, 3, 64, 64, 1, 1 << 56, 0.25, 1, 1, *b64, *tail, *ok, None) == -1  # pos0
    assert lib.vg_gather_degrade_u8_ex(*head, 5, 4, 16, 49, 16, 49, *tail, *ok, None) == -1             # max < min
    assert lib.vg_gather_degrade_u8_ex(*head, 1, 40, 16, 49, 16, 49, *tail, *ok, None) == -1            # empty x range
    assert lib.vg_gather_degrade_u8_ex(*head, *b64, buf, buf, buf, 2, 1, *ok, None) == -1               # CP < C
    assert lib.vg_gather_degrade_u8_ex(*head, *b64, buf, buf, buf, 8, 7, *ok, None) == -3               # unknown dtype
    assert lib.vg_gather_degrade_u8_ex(*head, *b64, buf, buf, ctypes.c_void_p(260), 8, 1, *ok, None) == -2   # NHWC alignment
    assert lib.vg_degrade_params_ex(1, 0, 0, 0.25, 1, 64, 64, *b64, buf, *ok, None) == -1               # B == 0
    assert lib.vg_degrade_params_ex(1, 0, 4, 0.25, 1, 64, 64, *b64, None, *ok, None) == -1              # out NULL
    assert lib.vg_degrade_params_ex(1, 0, 4, 0.25, 1, 64, 64, 1, 40, 16, 49, 16, 49, buf, *ok, None) == -1   # empty x range
    assert lib.vg_degrade_params_ex(1, 0, 4, 0.25, 1, 32, 32, *b64, buf, *ok, None) == -1               # rectangle outside
    assert lib.vg_degrade_params_ex(1, 1 << 56, 4, 0.25, 1, 64, 64, *b64, buf, *ok, None) == -1         # position 2^56
    # the median filter
    x, y = ctypes.c_void_p(1 << 20), ctypes.c_void_p(2 << 20)
    assert lib.vg_median_filter(None, y, 2, 3, 8, 8, 1, None) == -1
    assert lib.vg_median_filter(x, None, 2, 3, 8, 8, 1, None) == -1
    assert lib.vg_median_filter(x, x, 2, 3, 8, 8, 1, None) == -1                                        # x == y
    assert lib.vg_median_filter(x, ctypes.c_void_p((1 << 20) + 64), 2, 3, 8, 8, 1, None) == -1          # overlapping
    for r in (-1, 0, 3):
        assert lib.vg_median_filter(x, y, 2, 3, 8, 8, r, None) == -1, r
    assert lib.vg_median_filter(x, y, 2, 3, 1, 8, 1, None) == -1                                        # min(H, W) < r + 1
    assert lib.vg_median_filter(x, y, 2, 3, 8, 2, 2, None) == -1
    for B, C, H, W in ((0, 3, 8, 8), (2, 0, 8, 8), (2, 3, 0, 8), (2, 3, 8, 0), (1 << 16, 1 << 8, 1 << 4, 1 << 4)):
        assert lib.vg_median_filter(x, y, B, C, H, W, 1, None) == -1, (B, C, H, W)
    assert lib.vg_median_filter(ctypes.c_void_p((1 << 20) + 2), y, 2, 3, 8, 8, 1, None) == -2           # not 4-byte aligned
    assert lib.vg_median_filter(x, ctypes.c_void_p((2 << 20) + 1), 2, 3, 8, 8, 1, None) == -2


# ---- the Python surface ----------------------------------------------------------------------------------------------------------
def test_degrade_validation_and_repr():
    d = data.Degrade(0.25)
    assert (d.noise_model, d.impulse_max_p, d.salt_ratio, d.pure_gaussian) == ("gaussian", 0.0, 0.5, True)
    assert repr(d) == "Degrade(noise_max_std=0.25, rect=True, normalize=True)"       # the defaults do not show
    d = data.Degrade(0.25, False, True, "shot", 0.1, 0.25)
    assert (d.noise_model, d.impulse_max_p, d.salt_ratio, d.pure_gaussian, d.pairs) == ("shot", 0.1, 0.25, False, True)
    assert repr(d) == "Degrade(noise_max_std=0.25, rect=False, normalize=True, noise_model='shot', impulse_max_p=0.1, salt_ratio=0.25)"
    assert repr(data.Degrade(0.1, noise_model="speckle")).endswith("normalize=True, noise_model='speckle')")
    assert not data.Degrade(0.1, impulse_max_p=0.2).pure_gaussian
    for kw, word in ((dict(noise_model="poisson"), "poisson"), (dict(noise_model=1), "1"), (dict(impulse_max_p=-0.1), "-0.1"),
                     (dict(impulse_max_p=1.5), "1.5"), (dict(impulse_max_p=math.nan), "nan"), (dict(salt_ratio=2), "2"),
                     (dict(salt_ratio="half"), "half"), (dict(impulse_max_p=True), "True")):
        with pytest.raises(ValueError, match=re.escape(word)):
            data.Degrade(0.25, **kw)
    with pytest.raises(ValueError, match="laplace"):
        data.get_dataset_loaders("/nonexistent", noise_max_std=0.2, noise_model="laplace")   # refused before any decoding


def test_median_and_make_baseline_validation():
    m = baselines.Median()
    assert m.radius == 1 and m.needs_rects is False and m.name == "median"
    assert baselines.Median(2).radius == 2
    for bad in (0, 3, 1.0, True, "1", None):
        with pytest.raises(ValueError):
            baselines.Median(bad)
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 1, 4, 4))                                       # there is no CPU path
    mk = baselines.make_baseline
    assert mk("t", None) is None and mk("t", m) is m
    assert isinstance(mk("t", "median"), baselines.Median) and mk("t", "median").radius == 1
    assert mk("t", {"radius": 2}).radius == 2
    assert isinstance(mk("t", "median", allow_oracle=False), baselines.Median)
    nlm = mk("t", "nlm")
    assert isinstance(nlm, baselines.NLMeans) and nlm.name == "nlm" and nlm.sigma == "oracle"
    assert mk("t", {"sigma": "estimate"}).sigma == "estimate"
    for bad in ("mean", 3, {"radius": 5}, {"radius": 1, "sigma": 0.1}, {"search": 1}):
        with pytest.raises(ValueError):
            mk("t", bad)
    V = import_module(PKG)
    assert V.Median is baselines.Median and "Median" in V.__all__


class _Loader:
    def __init__(self, degrade):
        self.degrade = degrade


def test_oracle_sigma_is_refused_unless_the_loader_is_pure_gaussian():
    denoise = import_module(PKG + ".denoise")
    oracle, blind = baselines.NLMeans(), baselines.NLMeans(sigma="estimate")
    check = baselines.check_oracle_sigma
    for d in (data.Degrade(0.2, noise_model="speckle"), data.Degrade(0.2, noise_model="shot"), data.Degrade(0.2, impulse_max_p=0.1)):
        with pytest.raises(ValueError, match="column 1") as e:
            check("paired_test_epoch", oracle, _Loader(d))
        assert "not a Gaussian sigma" in str(e.value) and "'estimate'" in str(e.value) and "number" in str(e.value)
        check("paired_test_epoch", blind, _Loader(d))
        check("paired_test_epoch", baselines.NLMeans(sigma=0.1), _Loader(d))
        check("paired_test_epoch", baselines.Median(), _Loader(d))
        # the pass itself refuses before it touches the networks or the loader
        with pytest.raises(ValueError, match="column 1"):
            denoise.paired_test_epoch(None, None, _Loader(d), baseline="nlm")
    check("paired_test_epoch", oracle, _Loader(data.Degrade(0.2)))         # the default Degrade: nothing changes
    check("paired_test_epoch", oracle, [("noisy", "clean")])               # a plain iterable has no Degrade
    check("paired_test_epoch", None, _Loader(data.Degrade(0.2, noise_model="shot")))


def test_new_symbols_are_declared_bound_and_exported_with_the_abi_still_at_31():
    L = import_module(PKG + "._lib")
    lib = L.load()
    src = open(os.path.join(ROOT, "include", "vaegan_hip.h")).read()
    assert int(re.search(r"#define\s+VG_ABI_VERSION\s+(\d+)", src).group(1)) == L.ABI_VERSION == 31
    assert lib.vg_abi_version() == 31
    for name in ("vg_gather_degrade_u8_ex", "vg_degrade_params_ex", "vg_median_filter"):
        assert name in L.SIGNATURES and re.search(r"\b%s\s*\(" % name, src), name
        assert getattr(lib, name) is not None
    ids = P.header_draw_ids(src)
    assert ids["VG_DRAW_DEGRADE_IMPULSE"] == R.DRAW_IMPULSE == 19 and ids["VG_DRAW_DEGRADE_SALT"] == R.DRAW_SALT == 20
    assert len(set(ids.values())) == len(ids)
    for name, v in (("VG_NOISE_GAUSSIAN", 0), ("VG_NOISE_SPECKLE", 1), ("VG_NOISE_SHOT", 2)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, src).group(1)) == getattr(L, name) == v == R.KINDS[name[9:].lower()]
    ops = import_module(PKG + ".ops")
    assert callable(ops.median_filter) and ops.NOISE_KIND == R.KINDS
    assert (ops.DRAW_DEGRADE_IMPULSE, ops.DRAW_DEGRADE_SALT) == (19, 20)
