"""CPU: the spectral generation metric without a GPU.  (1) spectrum.py's tables against independent forms: the DFT tables
applied as matrices against np.fft.rfft2, the window against scipy, the integer bin rule against a Fraction evaluation of
its definition, the weights and Parseval; (2) metrics.spectral_distance against hand-computed profiles; (3) what the metric
is FOR: a +-0.02 checkerboard that SSIM does not see lifts the last radial bin by more than 10 dB; (4) the exact-input
table of the GPU tests: every intermediate below 2^53, and every row tells a correct kernel from four wrong ones; (5) the
C ABI's host checks and the Python surface's loud failures.  tests/_spectrum_ref.py shares no code with spectrum.py."""
import ctypes
import os
import re
from importlib import import_module

import numpy as np
import pytest
import torch

import _spectrum_ref as R
import vaegan_amd as V

PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = import_module(PKG + ".spectrum")
M = import_module(PKG + ".metrics")
U = R.U

SIZES = ((5, 7), (16, 16), (17, 16), (33, 17), (64, 96), (65, 65), (256, 256))


def plan_tabs(p):
    return p.tw_re, p.tw_im, p.th_re, p.th_im, p.weight


# ---- 1: the plan's tables ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", ((5, 7), (16, 16), (17, 16), (33, 17), (64, 96), (65, 65)))
@pytest.mark.parametrize("win", ("hann", "none"))
def test_tables_applied_as_matrices_equal_rfft2(H, W, win):
    """Z = th (x tw) against np.fft.rfft2(x w_H w_W).  Bound, counted: an element of Z is a sum of W products followed by a
    sum of H products, (H + W) roundings of products and as many of additions folded into gamma_(H+W); each table entry
    carries 1 u from its evaluation and 1 u from its window product, two tables: (H + W + 4) u against sum |th| |x| |tw|;
    doubled, the FFT being f64 arithmetic of the same class."""
    p = S.spectrum_plan(H, W, window=win)
    x = np.random.default_rng(H * 1000 + W).uniform(-1, 1, (H, W))
    tw, th = p.tw_re + 1j * p.tw_im, p.th_re + 1j * p.th_im
    Z = th @ (x @ tw)
    want = np.fft.rfft2(x * R.window(H, win)[:, None] * R.window(W, win)[None, :])
    bound = 2 * (H + W + 4) * U * (np.abs(th) @ (np.abs(x) @ np.abs(tw)))
    err = np.abs(Z - want)
    print(f"rfft2 {H}x{W} {win}: max err / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("N", (2, 5, 7, 16, 17, 33, 64, 65, 96, 256))
def test_window_equals_scipy_periodic_hann_and_tables_are_exactly_symmetric(N):
    get_window = pytest.importorskip("scipy.signal").get_window
    w = S.window_table(N, "hann")
    assert np.abs(w - get_window("hann", N)).max() <= 4 * U          # both 0.5 - 0.5 cos: one cos (1 u), one fma each side
    assert (w[1:] == w[1:][::-1]).all() and w[0] == 0.0
    assert (S.window_table(N, "none") == 1.0).all()
    re, im = S.dft_table(N, N, "none", False)
    k = np.arange(N)
    assert (re == re[:, (-k) % N]).all() and (im == -im[:, (-k) % N]).all()          # Hermitian in y, bit for bit
    assert (re == re.T).all() and (im == im.T).all()
    # against the unreduced form, whose argument (up to 2 pi N) carries three roundings: pi, the product, the division
    assert np.abs(re + 1j * im - np.exp(-2j * np.pi * np.outer(k, k) / N)).max() <= 3 * 2 * np.pi * N * U + 4 * U
    if N % 4 == 0:
        assert re[1, N // 4] == 0.0 and im[1, N // 4] == -1.0 and re[1, N // 2] == -1.0 and im[1, N // 2] == 0.0


@pytest.mark.parametrize("H,W", SIZES)
def test_integer_bin_rule_equals_the_fraction_definition(H, W):
    Wh = W // 2 + 1
    sweep = sorted({1, 2, 3, min(H, W) // 2, min(H, W)}) if max(H, W) <= 96 else [min(H, W) // 2]
    for n_bins in sweep:
        p = S.spectrum_plan(H, W, n_bins, window="none")
        want = np.array([[R.radial_bin_fraction(H, W, n_bins, u, v) for v in range(Wh)] for u in range(H)])
        assert (p.bin_of == want).all(), n_bins
        order, start, counts = R.radial_csr(H, W, n_bins)
        assert (p.order == order).all() and (p.bin_start == start).all() and (p.counts == counts).all()
        assert p.order.dtype == np.int32 and p.bin_start.dtype == np.int32 and p.bin_start[-1] == H * Wh
    p = S.spectrum_plan(H, W)
    assert p.n_bins == min(H, W) // 2 and (p.counts > 0).all(), "an empty bin at the default n_bins"
    assert p.bin_of[(H // 2), W // 2] == p.n_bins - 1                                 # the Nyquist corner: the last bin
    assert p.weight.sum() == H * W and (p.weight == R.half_weight(H, W)).all()
    assert np.allclose(p.centers, (np.arange(p.n_bins) + 0.5) / p.n_bins * R.R_MAX)


def test_every_admitted_size_has_no_empty_bin_and_full_weight():
    """The sweep over sizes, at the default n_bins: cheap, the plan's own vectorised rule."""
    for H in list(range(2, 40)) + [63, 64, 65, 127, 128, 129, 255, 256]:
        for W in (2, 3, 4, 5, 8, 15, 16, 17, 31, 32, 33, 64, 65, 96, 128, 255, 256):
            bins = S.radial_bins(H, W, max(1, min(H, W) // 2))
            assert np.bincount(bins.reshape(-1), minlength=max(1, min(H, W) // 2)).min() > 0, (H, W)
            assert S.half_weight(H, W).sum() == H * W


@pytest.mark.parametrize("H,W", ((5, 7), (16, 16), (17, 16), (64, 96)))
def test_parseval(H, W):
    """sum weight P = H W sum x^2 for window='none', center=False: through the plan's tables and through the FFT."""
    p = S.spectrum_plan(H, W, window="none")
    x = np.random.default_rng(5).uniform(-1, 1, (2, 3, H, W)).astype(np.float32)
    want = H * W * (x.astype(np.float64) ** 2).sum(axis=(1, 2, 3))
    prof, P = R.profiles_generic(x, False, *plan_tabs(p), p.order, p.bin_start, p.n_bins)
    assert np.allclose(prof.sum(1), want, rtol=1e-12) and np.allclose((P * p.weight).sum((1, 2)), want, rtol=1e-12)
    assert np.allclose(R.profiles_fft(x, None, "none", False)[0].sum(1), want, rtol=1e-12)


def test_two_d_plan_is_the_identity_table():
    p = S.spectrum_plan(6, 9, bins="2d")
    assert p.n_bins == 6 * 5 and (p.order == np.arange(30)).all() and (p.bin_start == np.arange(31)).all()
    assert (p.counts == 1).all() and p.centers[0] == 0.0 and abs(p.centers[3 * 5 + 4] - np.hypot(3 / 6, 4 / 9)) < 1e-15
    o, s, _ = R.identity_csr(6, 9)
    assert (p.order == o).all() and (p.bin_start == s).all()


@pytest.mark.parametrize("H,W,C,center", ((16, 16, 1, True), (33, 17, 3, True), (64, 96, 3, False), (64, 64, 3, True)))
def test_the_two_restatements_agree_within_the_counted_bound(H, W, C, center):
    """The bound the GPU test uses must first hold between the FFT form and the matrix form on the CPU."""
    p = S.spectrum_plan(H, W)
    x = np.random.default_rng(H + W + C).uniform(-1, 1, (2, C, H, W)).astype(np.float32)
    a, Pa = R.profiles_fft(x, None, "hann", center)
    b, Pb = R.profiles_generic(x, center, *plan_tabs(p), p.order, p.bin_start, p.n_bins)
    bound, dP = R.profile_bound(x, center, *plan_tabs(p), p.order, p.bin_start, p.n_bins)
    print(f"fft vs matrices {H}x{W} C={C}: prof err/bound {(np.abs(a - b) / bound).max():.4f}, "
          f"map err/bound {(np.abs(Pa - Pb) / np.maximum(dP, 1e-300)).max():.4f}")
    assert (np.abs(a - b) <= bound).all() and (np.abs(Pa - Pb) <= dP).all()


# ---- 2: spectral_distance -------------------------------------------------------------------------------------------------
def _stats(plan, mean, n=4):
    st = M.SpectrumStats(plan, device="cpu")
    st.load_state_dict({"sum": torch.tensor(np.asarray(mean, np.float64) * n), "sumsq": torch.zeros(plan.n_bins, dtype=torch.float64),
                        "n": torch.tensor(n)})
    return st


def test_spectral_distance_on_hand_computed_profiles():
    p = S.spectrum_plan(16, 16, 8)
    mr = np.array([9.0, 100.0, 10.0, 10.0, 1.0, 1.0, 1.0, 1.0])
    mf = np.array([1.0, 10.0, 10.0, 100.0, 1.0, 1.0, 1.0, 10.0])
    d = V.spectral_distance(_stats(p, mr), _stats(p, mf))
    # bins 1 .. 7: ratios 10, 1, 1/10, 1, 1, 1, 1/10 -> 10 dB, 0, -10 dB, 0, 0, 0, -10 dB
    assert abs(d["lsd_db"] - np.sqrt(300.0 / 7.0)) < 1e-12 and d["bins_used"] == 7 and d["bins_skipped"] == 0
    # bins at or above half of r_max: 4 .. 7; the lowest bin is left out of the total
    assert abs(d["hf_share_real"] - 4.0 / 124.0) < 1e-15 and abs(d["hf_share_fake"] - 13.0 / 133.0) < 1e-15
    assert abs(d["hf_excess_db"] - 10 * np.log10((13.0 / 133.0) / (4.0 / 124.0))) < 1e-12
    assert (d["mean_real"] == mr).all() and (d["mean_fake"] == mf).all() and (d["centers"] == p.centers).all()
    ref = R.spectral_distance(mr, mf, p.counts, p.frac_lo)
    for k, v in ref.items():
        assert d[k] == pytest.approx(v, rel=1e-13), k
    # symmetric in dB
    e = V.spectral_distance(_stats(p, mf), _stats(p, mr))
    assert e["lsd_db"] == pytest.approx(d["lsd_db"], rel=1e-14) and e["hf_excess_db"] == pytest.approx(-d["hf_excess_db"], rel=1e-12)
    assert (e["hf_share_real"], e["hf_share_fake"]) == (d["hf_share_fake"], d["hf_share_real"])
    # identical statistics: exactly 0
    z = V.spectral_distance(_stats(p, mr), _stats(p, mr))
    assert z["lsd_db"] == 0.0 and z["hf_excess_db"] == 0.0
    # skip_bins and hf_from move the sets
    d0 = V.spectral_distance(_stats(p, mr), _stats(p, mf), skip_bins=0, hf_from=0.75)
    assert abs(d0["lsd_db"] - np.sqrt((300.0 + (10 * np.log10(9.0)) ** 2) / 8.0)) < 1e-12
    assert abs(d0["hf_share_real"] - 2.0 / 133.0) < 1e-15 and abs(d0["hf_share_fake"] - 11.0 / 134.0) < 1e-15


def test_spectral_distance_skips_and_counts_zero_bins():
    p = S.spectrum_plan(16, 16, 8)
    mr = np.array([1.0, 4.0, 0.0, 2.0, 1.0, 1.0, 1.0, 1.0])
    mf = np.array([1.0, 4.0, 3.0, 0.0, 1.0, 1.0, 1.0, 100.0])
    d = V.spectral_distance(_stats(p, mr), _stats(p, mf))
    assert d["bins_skipped"] == 2 and d["bins_used"] == 5 and abs(d["lsd_db"] - np.sqrt(400.0 / 5.0)) < 1e-12
    assert np.isfinite(d["hf_excess_db"])
    ref = R.spectral_distance(mr, mf, p.counts, p.frac_lo)
    assert ref["bins_skipped"] == 2 and d["lsd_db"] == pytest.approx(ref["lsd_db"], rel=1e-13)
    # a plan with an empty bin: n_bins = min(H, W) of a 2 x 2 image has 2 bins over 4 points; force one through a 2-d check
    q = S.spectrum_plan(4, 4, 4)
    live = int(((np.arange(4) >= 1) & (q.counts > 0)).sum())
    dq = V.spectral_distance(_stats(q, np.ones(4)), _stats(q, np.ones(4)))
    assert dq["bins_used"] == live and dq["lsd_db"] == 0.0


# ---- 3: what the metric is for --------------------------------------------------------------------------------------------
def test_a_checkerboard_ssim_does_not_see_lifts_the_last_bin():
    """S = 64, 128 images a side, smooth noise (R.smooth_images); +-0.02 of checkerboard.  Measured with this restatement: the
    last bin of the contaminated set stands 17.1 dB above the clean one (two independent clean sets differ by 0.05 dB there),
    lsd_db goes from 0.10 (two independent clean sets) to 3.07, and the oracle's SSIM between clean and contaminated images is
    0.9996."""
    import vaegan_ref as O
    n, Sz = 128, 64
    a, b = R.smooth_images(n, Sz, 1), R.smooth_images(n, Sz, 2)
    dirty = a + R.checkerboard(Sz)[None, None]
    ma, mb, md = (R.profiles_fft(s)[0].mean(0) for s in (a, b, dirty))
    lift = 10 * np.log10(md[-1] / ma[-1])
    clean = abs(10 * np.log10(mb[-1] / ma[-1]))
    p = S.spectrum_plan(Sz, Sz)
    lsd_clean = R.spectral_distance(ma, mb, p.counts, p.frac_lo)["lsd_db"]
    lsd_dirty = R.spectral_distance(ma, md, p.counts, p.frac_lo)["lsd_db"]
    ssim = O.ssim(torch.from_numpy(a[:32]), torch.from_numpy(dirty[:32]))
    print(f"last-bin lift {lift:.2f} dB (clean pair {clean:.2f} dB), lsd_db {lsd_clean:.2f} -> {lsd_dirty:.2f}, SSIM {ssim:.5f}")
    assert lift >= clean + 10.0
    assert lsd_dirty > lsd_clean
    assert ssim > 0.99
    d = M._spectral_distance(p, ma, md, 1, 0.5)
    assert d["lsd_db"] == pytest.approx(lsd_dirty, rel=1e-12) and d["hf_excess_db"] > 0.0


# ---- 4: the exact-input table ---------------------------------------------------------------------------------------------
EXACT_ROWS = [(H, W, 3, C, center) for (H, W) in R.EXACT_SHAPES for C in (1, 3) for center in (False, True)] + \
             [(256, 256, 1, 1, False)]


@pytest.mark.parametrize("H,W,B,C,center", EXACT_ROWS)
def test_exact_rows_stay_below_2_53_and_see_every_blind_spot(H, W, B, C, center):
    """The rows of the GPU exact table (B = 3 holds B = 1: images are independent).  profiles_generic(exact=True) asserts
    every intermediate below 2^53; here each row must also give a different answer under each single mistake."""
    x, tabs = R.exact_case(H, W, B, C, center, 100 * H + W)
    if center:
        assert all(R.contract_mean(pl) in (0.25, 1.0) for pl in x.reshape(-1, H, W)), "the mean must be a non-zero dyadic"
    kinds = R.BIN_KINDS if max(H, W) <= 128 else ("default",)
    for kind in kinds:
        order, start, n_bins = R.csr_of_kind(H, W, kind)
        prof, P = R.profiles_generic(x, center, *tabs, order, start, n_bins, exact=True)
        assert np.abs(prof).max() > 0 and (prof == np.rint(prof * 16) / 16).all()
        for name, (mt, ms) in R.mutations(tabs, order, start, n_bins).items():
            wrong, _ = R.profiles_generic(x, center, *mt, order, ms, n_bins)          # f64: enough to differ
            assert (wrong != prof).any(), (kind, name)
        if center:
            off, _ = R.profiles_generic(x, False, *tabs, order, start, n_bins)
            assert (off != prof).any(), (kind, "mean not subtracted")
        both, _ = R.profiles_generic(x, center, *tabs, order, start, n_bins)           # f64 agrees with the integers: exact
        assert (both == prof).all()


def test_table_safety_rules_of_the_restatement():
    """Out-of-range and negative entries are skipped; a bin whose bounds are not 0 <= s <= e <= nnz gives 0."""
    P = np.arange(1.0, 13.0).reshape(1, 12)
    w = np.full(12, 2.0)
    order = np.array([0, 5, -1, 12, 11, 3, 99, 7], np.int32)
    assert (R.bin_sum(P, w, order, np.array([0, 3, 8], np.int32), 2, 12) == [[2 * (1 + 6), 2 * (12 + 4 + 8)]]).all()
    assert (R.bin_sum(P, w, order, np.array([0, 5, 3, 8], np.int32), 3, 12) == [[2 * (1 + 6 + 12), 0, 2 * (12 + 4 + 8)]]).all()
    assert (R.bin_sum(P, w, order, np.array([-1, 3, 8], np.int32), 2, 12) == [[0, 2 * (12 + 4 + 8)]]).all()    # s = -1
    assert (R.bin_sum(P, w, order, np.array([0, 3, 13], np.int32), 2, 12) == [[14, 0]]).all()      # nnz clamps to 12, e = 13 > 12
    assert (R.bin_sum(P, w, order, np.array([0, 3, -5], np.int32), 2, 12) == [[0, 0]]).all()       # nnz clamps to 0


# ---- 5: the C ABI on the host, the Python surface --------------------------------------------------------------------------
def _ptrs():
    base = 1 << 24
    names = ("x", "tw_re", "tw_im", "th_re", "th_im", "weight", "order", "bin_start", "power", "prof", "ws")
    return {n: base + (i << 22) for i, n in enumerate(names)}          # 4 MiB apart: nothing overlaps at the sizes below


def _call(lib, p, B=2, C=3, H=16, W=16, center=1, n_bins=8, ws_bytes=1 << 20):
    v = ctypes.c_void_p
    return lib.vg_spectrum_profiles(v(p["x"]), B, C, H, W, center, v(p["tw_re"]), v(p["tw_im"]), v(p["th_re"]), v(p["th_im"]),
                                    v(p["weight"]), v(p["order"]), v(p["bin_start"]), n_bins, v(p["power"]), v(p["prof"]),
                                    v(p["ws"]), ws_bytes, None)


def test_c_abi_rejects_bad_spectrum_arguments_on_host():
    L = import_module(PKG + "._lib")
    lib = L.load()
    need = ctypes.c_int64(-7)
    assert lib.vg_spectrum_ws_bytes(2, 3, 16, 16, ctypes.byref(need)) == 0 and need.value == 8 * (2 * 3 + 2 * 16 * 9)
    assert lib.vg_spectrum_ws_bytes(32, 3, 256, 256, ctypes.byref(need)) == 0 and need.value == 8 * (96 + 32 * 256 * 129)
    assert lib.vg_spectrum_ws_bytes(1, 1, 5, 7, ctypes.byref(need)) == 0 and need.value == 8 * (1 + 5 * 4)
    assert lib.vg_spectrum_ws_bytes(2, 3, 16, 16, None) == -1
    for B, C, H, W in ((0, 3, 16, 16), (2, 0, 16, 16), (2, 5, 16, 16), (2, 3, 1, 16), (2, 3, 16, 1), (2, 3, 257, 16),
                       (2, 3, 16, 257), (1 << 20, 4, 256, 256)):
        assert lib.vg_spectrum_ws_bytes(B, C, H, W, ctypes.byref(need)) == -1, (B, C, H, W)
        assert _call(lib, _ptrs(), B=B, C=C, H=H, W=W, ws_bytes=1 << 40) == -1, (B, C, H, W)
    ok = _ptrs()
    for name in ok:
        if name == "power":
            continue                                                   # NULL power is a mode, not an error
        assert _call(lib, dict(ok, **{name: 0})) == -1, name
    for center in (-1, 2):
        assert _call(lib, ok, center=center) == -1
    for n_bins in (0, -1, 16 * 9 + 1):
        assert _call(lib, ok, n_bins=n_bins) == -1
    assert _call(lib, ok, ws_bytes=8 * (6 + 2 * 16 * 9) - 1) == -1                      # one byte short
    assert _call(lib, ok, ws_bytes=0) == -1
    # aliasing: every output against every input and against the other outputs
    for out in ("prof", "power", "ws"):
        for other in ok:
            if other != out:
                assert _call(lib, dict(ok, **{out: ok[other]})) == -1, (out, other)
    assert _call(lib, dict(ok, prof=ok["x"] + 2 * 3 * 16 * 16 * 4 - 8)) == -1           # the tail of x
    assert _call(lib, dict(ok, ws=ok["power"] + 2 * 16 * 9 * 8 - 8)) == -1              # the tail of the map
    # alignment
    for name in ("x", "order", "bin_start"):
        assert _call(lib, dict(ok, **{name: ok[name] + 2})) == -2, name
    for name in ("tw_re", "tw_im", "th_re", "th_im", "weight", "power", "prof", "ws"):
        assert _call(lib, dict(ok, **{name: ok[name] + 4})) == -2, name
    # the accumulator
    v = ctypes.c_void_p
    a, s, q = 1 << 24, 2 << 24, 3 << 24
    assert lib.vg_spectrum_accum(None, 2, 8, v(s), v(q), None) == -1
    assert lib.vg_spectrum_accum(v(a), 2, 8, None, v(q), None) == -1
    assert lib.vg_spectrum_accum(v(a), 2, 8, v(s), None, None) == -1
    for B, n in ((0, 8), (-1, 8), (2, 0), (2, 256 * 129 + 1), (1 << 20, 1 << 12)):
        assert lib.vg_spectrum_accum(v(a), B, n, v(s), v(q), None) == -1, (B, n)
    assert lib.vg_spectrum_accum(v(a), 2, 8, v(s), v(s), None) == -1
    assert lib.vg_spectrum_accum(v(a), 2, 8, v(a + 64), v(q), None) == -1
    assert lib.vg_spectrum_accum(v(a), 2, 8, v(s), v(s + 56), None) == -1
    for bad in ((a + 4, s, q), (a, s + 4, q), (a, s, q + 4)):
        assert lib.vg_spectrum_accum(v(bad[0]), 2, 8, v(bad[1]), v(bad[2]), None) == -2


def test_plan_validation():
    for bad in (dict(H=1), dict(W=1), dict(H=257), dict(W=300), dict(H=16.0), dict(H=True), dict(n_bins=0), dict(n_bins=17),
                dict(n_bins=2.5), dict(n_bins=True), dict(window="hamming"), dict(bins="polar"), dict(bins="2d", n_bins=7)):
        kw = dict(H=16, W=24)
        kw.update(bad)
        with pytest.raises(RuntimeError, match="spectrum_plan"):
            S.spectrum_plan(**kw)
    p = S.spectrum_plan(16, 24)
    assert (p.H, p.W, p.Wh, p.n_bins, p.window, p.bins) == (16, 24, 13, 8, "hann", "radial")
    assert S.spectrum_plan(16, 24, 16).n_bins == 16 and S.spectrum_plan(16, 24, bins="2d", n_bins=16 * 13).n_bins == 208
    assert repr(p) == "SpectrumPlan(H=16, W=24, n_bins=8, window='hann', bins='radial')"
    assert p.flops(3) == 2.0 * 3 * 16 * 24 * 13 * (2 + 4 * 16 / 24)
    for name in S.SpectrumPlan.TABLES:
        t = getattr(p, name)
        assert t.flags["C_CONTIGUOUS"] and t.dtype == (np.int32 if name in ("order", "bin_start") else np.float64), name
    assert p.same_bins(S.spectrum_plan(16, 24)) and not p.same_bins(S.spectrum_plan(16, 24, window="none"))


def test_spectrum_stats_holds_state_on_the_cpu_and_fails_loudly():
    p = S.spectrum_plan(16, 16)
    st = M.SpectrumStats(p, device="cpu")
    assert V.SpectrumStats is M.SpectrumStats and st.n == 0 and st.sum.dtype == torch.float64 and tuple(st.sumsq.shape) == (8,)
    with pytest.raises(RuntimeError, match="MI355X"):
        st.update(torch.zeros(2, 3, 16, 16))
    with pytest.raises(RuntimeError, match="no image yet"):
        st.mean_profile()
    with pytest.raises(RuntimeError, match="at least two"):
        st.var_profile()
    with pytest.raises(RuntimeError, match="SpectrumPlan"):
        M.SpectrumStats((16, 16), device="cpu")
    with pytest.raises(RuntimeError, match="center"):
        M.SpectrumStats(p, device="cpu", center=1)
    prof = np.array([[1.0, 2, 3, 4, 5, 6, 7, 8], [3.0, 2, 1, 0, 1, 2, 3, 4], [2.0, 2, 2, 2, 2, 2, 2, 2]])
    st.load_state_dict({"sum": torch.tensor(prof.sum(0)), "sumsq": torch.tensor((prof ** 2).sum(0)), "n": torch.tensor(3)})
    assert np.allclose(st.mean_profile(), prof.mean(0)) and np.allclose(st.var_profile(), prof.var(0, ddof=1))
    other = M.SpectrumStats(p, device="cpu").load_state_dict(st.state_dict())
    assert other.n == 3 and torch.equal(other.sum, st.sum) and other.sum.data_ptr() != st.sum.data_ptr()
    other.merge(st)
    assert other.n == 6 and torch.equal(other.sum, 2 * st.sum) and torch.equal(other.sumsq, 2 * st.sumsq)
    with pytest.raises(RuntimeError, match="plans differ"):
        other.merge(M.SpectrumStats(S.spectrum_plan(16, 16, 4), device="cpu"))
    with pytest.raises(RuntimeError, match="f64"):
        st.load_state_dict({"sum": torch.zeros(8), "sumsq": torch.zeros(8, dtype=torch.float64), "n": torch.tensor(1)})
    with pytest.raises(RuntimeError, match="f64"):
        st.load_state_dict({"sum": torch.zeros(7, dtype=torch.float64), "sumsq": torch.zeros(8, dtype=torch.float64), "n": torch.tensor(1)})
    with pytest.raises(RuntimeError, match="SpectrumStats"):
        V.spectral_distance(st, prof)
    with pytest.raises(RuntimeError, match="plans differ"):
        V.spectral_distance(st, M.SpectrumStats(S.spectrum_plan(16, 16, 4), device="cpu"))
    with pytest.raises(RuntimeError, match="at least one image"):
        V.spectral_distance(st, M.SpectrumStats(p, device="cpu"))
    for kw in (dict(skip_bins=-1), dict(skip_bins=8), dict(skip_bins=1.0), dict(hf_from=1.5), dict(hf_from=-0.1)):
        with pytest.raises(RuntimeError, match="spectral_distance"):
            V.spectral_distance(st, other, **kw)


def test_ops_and_generation_pass_reject_what_they_do_not_take():
    ops = import_module(PKG + ".ops")
    p = S.spectrum_plan(16, 16)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.spectrum_profiles(torch.zeros(1, 1, 16, 16), p)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.spectrum_accum(torch.zeros(1, 8, dtype=torch.float64), torch.zeros(8, dtype=torch.float64),
                           torch.zeros(8, dtype=torch.float64))
    with pytest.raises(TypeError, match="unknown keyword"):
        V.evaluate_generation_spectrum(None, [], ndb_bins=3)
    with pytest.raises(RuntimeError, match="window"):
        V.evaluate_generation_spectrum(None, [], window="hamming")
    for bad in (0, -3, 2.0, True):
        with pytest.raises(RuntimeError, match="spectrum_bins"):
            V.evaluate_generation_spectrum(None, [], spectrum_bins=bad)


def test_new_symbols_are_declared_bound_and_exported_with_the_abi_still_at_31():
    import inspect
    L = import_module(PKG + "._lib")
    lib = L.load()
    src = open(os.path.join(ROOT, "include", "vaegan_hip.h")).read()
    assert int(re.search(r"#define\s+VG_ABI_VERSION\s+(\d+)", src).group(1)) == L.ABI_VERSION == 31
    assert lib.vg_abi_version() == 31
    for name in ("vg_spectrum_ws_bytes", "vg_spectrum_profiles", "vg_spectrum_accum"):
        assert name in L.SIGNATURES and re.search(r"\b%s\s*\(" % name, src), name
        assert getattr(lib, name) is not None
    for name in ("spectrum", "SpectrumStats", "spectral_distance", "evaluate_generation_spectrum"):
        assert name in V.__all__ and hasattr(V, name) and name in V.__doc__, name
    assert V.spectrum is S and V.spectral_distance is M.spectral_distance
    assert V.evaluate_generation_spectrum is V.latent.evaluate_generation_spectrum
    ops = import_module(PKG + ".ops")
    assert callable(ops.spectrum_profiles) and callable(ops.spectrum_accum)
    # the pinned keyword list of evaluate_generation is untouched; the private pass takes the option last, default off
    assert "spectrum_bins" not in inspect.signature(V.evaluate_generation).parameters
    last = list(inspect.signature(V.latent._evaluate_generation).parameters.values())[-1]
    assert last.name == "spectrum" and last.default is None
