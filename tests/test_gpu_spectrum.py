"""GPU: the spectral generation metric (vg_spectrum_profiles, vg_spectrum_accum, csrc/spectrum.hip; spectrum.spectrum_plan,
metrics.SpectrumStats / spectral_distance, evaluate_generation_spectrum) against tests/_spectrum_ref.py: bit for bit on the
exact-input table (integer images and tables, every intermediate below 2^53, tests/test_spectrum_cpu.py shows that each row
sees a swapped re / im, a transposed table, a dropped weight, an off-by-one bin and a forgotten mean), within a counted
bound on random images with real DFT tables, and the layers above against loops written from public pieces."""
from importlib import import_module

import numpy as np
import pytest
import torch

import _spectrum_ref as R
import vaegan_amd as V
from test_gpu_parity import build

pytestmark = pytest.mark.gpu
DEV = "cuda"
PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
ops = import_module(PKG + ".ops")
L = import_module(PKG + "._lib")
S = import_module(PKG + ".spectrum")
M = import_module(PKG + ".metrics")
latent = import_module(PKG + ".latent")
U = R.U
GUARD = 64                                                   # sentinel doubles on either side of every output


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.int64)


def same_bits(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    return np.array_equal(bits(got), bits(want))


def guarded(n):
    """(buffer, view): n NaN doubles between two runs of GUARD sentinels."""
    buf = torch.full((n + 2 * GUARD,), -12345.0, dtype=torch.float64, device=DEV)
    buf[GUARD:GUARD + n] = float("nan")
    return buf, buf[GUARD:GUARD + n]


def guards_intact(buf):
    return bool((buf[:GUARD] == -12345.0).all() and (buf[-GUARD:] == -12345.0).all())


def dev_x(x, misalign=False):
    """x f32 on the device; misalign: its base 4 bytes past a 16-byte boundary."""
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32))
    if not misalign:
        return t.to(DEV)
    buf = torch.full((t.numel() + 8,), float("nan"), dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def dev_tabs(tabs):
    return [torch.from_numpy(np.ascontiguousarray(t, np.float64)).to(DEV) for t in tabs]


def raw(x, center, dtabs, order, start, n_bins, want_power):
    """One call of the C entry point over NaN-filled, guarded prof, power and ws -> (prof, power or None) as numpy."""
    B, C, H, W = x.shape
    Wh = W // 2 + 1
    need = L.c_int64(0)
    L.check(L.load().vg_spectrum_ws_bytes(B, C, H, W, L.byref(need)), "vg_spectrum_ws_bytes")
    assert need.value == 8 * (B * C + B * H * Wh)
    gp, prof = guarded(B * n_bins)
    gw, ws = guarded(need.value // 8)
    gm, power = guarded(B * H * Wh) if want_power else (None, None)
    o = torch.from_numpy(np.ascontiguousarray(order, np.int32)).to(DEV)
    s = torch.from_numpy(np.ascontiguousarray(start, np.int32)).to(DEV)
    rc = L.load().vg_spectrum_profiles(x.data_ptr(), B, C, H, W, int(center), *(t.data_ptr() for t in dtabs), o.data_ptr(),
                                       s.data_ptr(), n_bins, L.ptr(power), prof.data_ptr(), ws.data_ptr(), need.value,
                                       L.stream_ptr())
    L.check(rc, "vg_spectrum_profiles")
    torch.cuda.synchronize()
    assert guards_intact(gp) and guards_intact(gw) and (gm is None or guards_intact(gm)), "a write outside an output"
    if not want_power:                                       # the map then lives in ws, behind the plane means
        assert not torch.isnan(ws[B * C:]).any()
    return prof.cpu().numpy().reshape(B, n_bins), (power.cpu().numpy().reshape(B, H, Wh) if want_power else None)


# ---- the exact table ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", R.EXACT_SHAPES)
def test_exact_table_bit_for_bit(H, W):
    """B in {1, 3} x C in {1, 3} x n_bins in {1, 2, default, H Wh identity} x center x with / without power.  B = 1 is the
    first image of the B = 3 case (x base misaligned there): its expected profile is row 0 of the restatement's."""
    for C in (1, 3):
        for center in (False, True):
            x, tabs = R.exact_case(H, W, 3, C, center, 100 * H + W)
            dtabs = dev_tabs(tabs)
            x3, x1 = dev_x(x), dev_x(x[:1], misalign=True)
            for kind in R.BIN_KINDS:
                order, start, n_bins = R.csr_of_kind(H, W, kind)
                want, wantP = R.profiles_generic(x, center, *tabs, order, start, n_bins, exact=True)
                for want_power in (False, True):
                    for xd, b in ((x3, 3), (x1, 1)):
                        prof, power = raw(xd, center, dtabs, order, start, n_bins, want_power)
                        assert same_bits(prof, want[:b]), (C, center, kind, want_power, b)
                        assert power is None or same_bits(power, wantP[:b]), (C, center, kind, b)


def test_exact_largest_shape_bit_for_bit():
    x, tabs = R.exact_case(256, 256, 1, 1, False, 25600)
    order, start, n_bins = R.csr_of_kind(256, 256, "default")
    want, wantP = R.profiles_generic(x, False, *tabs, order, start, n_bins, exact=True)
    prof, power = raw(dev_x(x), False, dev_tabs(tabs), order, start, n_bins, True)
    assert same_bits(prof, want) and same_bits(power, wantP)


def test_table_safety():
    """Out-of-range and negative order entries, bins whose bounds are not 0 <= s <= e <= nnz: the result is the restatement
    that skips them, nothing outside the outputs is written (raw() checks the guards)."""
    H, W, B, C = 17, 16, 2, 3
    HWh = H * (W // 2 + 1)
    x, tabs = R.exact_case(H, W, B, C, True, 77)
    dtabs, xd = dev_tabs(tabs), dev_x(x)
    good, start, n_bins = R.csr_of_kind(H, W, "default")
    bad = good.copy()
    bad[[0, 5, 40, 77, HWh - 1]] = [-1, HWh, 2 ** 31 - 1, -2 ** 31, HWh + 5]
    bad[100:110] = -7
    cases = [(bad, start, n_bins)]
    for edit in ({3: 60, 4: 20}, {0: -4}, {n_bins: HWh + 1}, {n_bins: 2 ** 31 - 1}, {n_bins: -1}, {2: 2 ** 30}, {n_bins: 90}):
        s = start.copy()
        for k, v in edit.items():
            s[k] = v
        cases.append((bad, s, n_bins))
    one = np.array([5, HWh - 3], np.int32)
    cases.append((bad, one, 1))
    cases.append((np.full(HWh, 2 ** 30, np.int32), start, n_bins))                       # nothing in range: all zeros
    for order, s, nb in cases:
        want, _ = R.profiles_generic(x, True, *tabs, order, s, nb, exact=True)
        prof, _ = raw(xd, True, dtabs, order, s, nb, False)
        assert same_bits(prof, want), (s[:6], nb)
    # the thread-per-bin form of short bins: the identity table with holes
    ido, ids, idn = R.csr_of_kind(H, W, "identity")
    ido = ido.copy()
    ido[[1, 7, 50]] = [-1, HWh, 2 ** 31 - 1]
    ids = ids.copy()
    ids[10], ids[11] = 12, 9
    want, _ = R.profiles_generic(x, True, *tabs, ido, ids, idn, exact=True)
    assert (want[:, [1, 7, 50, 10]] == 0).all() and np.count_nonzero(want) > idn          # bin 10 is [12, 9): empty
    prof, _ = raw(xd, True, dtabs, ido, ids, idn, True)
    assert same_bits(prof, want)


# ---- random images ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,B,C", ((16, 16, 3, 3), (33, 17, 2, 1), (64, 64, 4, 3), (64, 96, 2, 3), (128, 128, 2, 3),
                                     (256, 256, 1, 2)))
def test_random_images_within_the_counted_bound_repeatable_and_independent(H, W, B, C):
    """Real DFT tables, images uniform in [-1, 1].  The bound is R.profile_bound: counted, not fitted, and checked between
    the two restatements on the CPU first (tests/test_spectrum_cpu.py)."""
    p = S.spectrum_plan(H, W)
    tabs = (p.tw_re, p.tw_im, p.th_re, p.th_im, p.weight)
    x = np.random.default_rng(H * 7 + W).uniform(-1, 1, (B, C, H, W)).astype(np.float32)
    xd = torch.from_numpy(x).to(DEV)
    for center in (True, False):
        want, wantP = R.profiles_generic(x, center, *tabs, p.order, p.bin_start, p.n_bins)
        bound, dP = R.profile_bound(x, center, *tabs, p.order, p.bin_start, p.n_bins)
        prof, power = ops.spectrum_profiles(xd, p, center=center, want_power=True)
        prof, power = prof.cpu().numpy(), power.cpu().numpy()
        ep, em = np.abs(prof - want) / bound, np.abs(power - wantP) / np.maximum(dP, 1e-300)
        print(f"{H}x{W} B={B} C={C} center={center}: profile err/bound {ep.max():.4f}, map err/bound {em.max():.4f}")
        assert (ep <= 1).all() and (em <= 1).all()
        again = ops.spectrum_profiles(xd, p, center=center)
        assert same_bits(again, prof), "the same call twice"
        solo = ops.spectrum_profiles(xd[B - 1:].contiguous(), p, center=center)
        assert same_bits(solo, prof[B - 1:]), "row b of a batch is the single-image call"
    if (H, W) == (64, 64):                                     # the FFT form, the 2-d table and the window switch
        fft, _ = R.profiles_fft(x, None, "hann", True)
        got = ops.spectrum_profiles(xd, p).cpu().numpy()
        assert (np.abs(got - fft) <= R.profile_bound(x, True, *tabs, p.order, p.bin_start, p.n_bins)[0]).all()
        p2 = S.spectrum_plan(H, W, bins="2d", window="none")
        got2, pw2 = ops.spectrum_profiles(xd, p2, center=False, want_power=True)
        assert same_bits(got2.view(B, H, p2.Wh), (pw2 * torch.from_numpy(p2.weight).to(DEV)).cpu().numpy())
        tot = (x.astype(np.float64) ** 2).sum((1, 2, 3)) * H * W                       # Parseval
        assert np.allclose(got2.sum(1).cpu().numpy(), tot, rtol=1e-12)


def test_op_wrappers_reject_what_the_kernels_do_not_take():
    p = S.spectrum_plan(16, 16)
    x = torch.zeros(2, 3, 16, 16, device=DEV)
    for bad, match in ((x.double(), "f32"), (x[0], "f32"), (torch.zeros(2, 3, 16, 17, device=DEV), "16 x 16"),
                       (torch.zeros(2, 5, 16, 16, device=DEV), "C <= 4"), (torch.zeros(0, 3, 16, 16, device=DEV), "B >= 1"),
                       (x.permute(0, 1, 3, 2), "contiguous")):
        with pytest.raises(RuntimeError, match=match):
            ops.spectrum_profiles(bad, p)
    with pytest.raises(RuntimeError, match="SpectrumPlan"):
        ops.spectrum_profiles(x, (16, 16))
    with pytest.raises(RuntimeError, match="bools"):
        ops.spectrum_profiles(x, p, center=1)
    s, q = torch.zeros(8, dtype=torch.float64, device=DEV), torch.zeros(8, dtype=torch.float64, device=DEV)
    prof = torch.ones(2, 8, dtype=torch.float64, device=DEV)
    for args in ((prof.float(), s, q), (prof[0], s, q), (prof, s[:7], q), (prof, s.float(), q), (prof, s, q.cpu())):
        with pytest.raises(RuntimeError):
            ops.spectrum_accum(*args)
    assert ops.spectrum_accum(prof[:0], s, q)[0] is s and not s.any()                  # b = 0: nothing happens


# ---- the accumulator --------------------------------------------------------------------------------------------------------
def test_accum_is_the_ascending_b_loop():
    g = np.random.default_rng(3)
    for n_bins in (1, 8, 300):
        chunks = [g.integers(-1000, 1000, size=(b, n_bins)).astype(np.float64) for b in (3, 0, 5, 1, 64)]
        s = torch.full((n_bins,), 7.0, dtype=torch.float64, device=DEV)
        q = torch.full((n_bins,), -3.0, dtype=torch.float64, device=DEV)
        ws, wq = np.full(n_bins, 7.0), np.full(n_bins, -3.0)
        for c in chunks:                                        # ragged updates, b = 0 among them
            ops.spectrum_accum(torch.from_numpy(c).to(DEV), s, q)
            ws, wq = R.accum(c, ws, wq)
        assert same_bits(s, ws) and same_bits(q, wq), n_bins
    chunks = [g.standard_normal((b, 40)) * 10.0 ** g.uniform(-3, 3, size=(1, 40)) for b in (7, 0, 33, 2)]
    s = torch.zeros(40, dtype=torch.float64, device=DEV)
    q = torch.zeros(40, dtype=torch.float64, device=DEV)
    for c in chunks:
        ops.spectrum_accum(torch.from_numpy(c).to(DEV), s, q)
    allp = np.concatenate(chunks)
    n_add = allp.shape[0]
    es = np.abs(s.cpu().numpy() - allp.sum(0)) / (2 * U * n_add * np.abs(allp).sum(0))
    eq = np.abs(q.cpu().numpy() - (allp ** 2).sum(0)) / (2 * U * n_add * (allp ** 2).sum(0))
    print(f"accum: sum err/bound {es.max():.4f}, sumsq err/bound {eq.max():.4f} (2 u per addition, {n_add} additions)")
    assert (es <= 1).all() and (eq <= 1).all()


# ---- SpectrumStats ----------------------------------------------------------------------------------------------------------
def test_spectrum_stats_update_merge_and_state_dict_round_trip():
    p = S.spectrum_plan(32, 32)
    x = np.random.default_rng(9).uniform(-1, 1, (11, 3, 32, 32)).astype(np.float32)
    xd = torch.from_numpy(x).to(DEV)
    prof, _ = R.profiles_generic(x, True, p.tw_re, p.tw_im, p.th_re, p.th_im, p.weight, p.order, p.bin_start, p.n_bins)
    st = M.SpectrumStats(p)
    for lo, hi in ((0, 4), (4, 4), (4, 5), (5, 11)):            # ragged, b = 0 among them
        assert st.update(xd[lo:hi]) is st
    assert st.n == 11
    dev_prof = ops.spectrum_profiles(xd, p)
    ws, wq = R.accum(dev_prof.cpu().numpy(), np.zeros(p.n_bins), np.zeros(p.n_bins))
    assert same_bits(st.sum, ws)                                # the device's own profiles, added in ascending order
    # the squares enter by fma on the device and by a product and a sum here: 2 u per addition
    assert (np.abs(st.sumsq.cpu().numpy() - wq) <= 2 * U * 11 * wq).all()
    assert np.allclose(st.mean_profile(), prof.mean(0), rtol=1e-10) and np.allclose(st.var_profile(), prof.var(0, ddof=1), rtol=1e-8)
    a, b = M.SpectrumStats(p).update(xd[:6]), M.SpectrumStats(p).update(xd[6:])
    sa, qa = a.sum.clone(), a.sumsq.clone()
    assert a.merge(b) is a and a.n == 11
    assert torch.equal(a.sum, sa + b.sum) and torch.equal(a.sumsq, qa + b.sumsq)
    assert np.allclose(a.mean_profile(), st.mean_profile(), rtol=1e-13)
    host = M.SpectrumStats(p, device="cpu").load_state_dict({k: v.cpu() for k, v in st.state_dict().items()})
    assert host.n == 11 and not host.sum.is_cuda and same_bits(host.sum, ws)
    with pytest.raises(RuntimeError, match="MI355X"):
        host.update(xd[:1])
    back = M.SpectrumStats(p).load_state_dict(host.state_dict())
    assert back.sum.is_cuda and back.n == 11 and torch.equal(back.sum, st.sum) and torch.equal(back.sumsq, st.sumsq)
    assert V.spectral_distance(st, back)["lsd_db"] == 0.0
    assert V.spectral_distance(host, back)["lsd_db"] == 0.0     # a CPU side holds state: the distance is host work
    with pytest.raises(RuntimeError, match="32, 32"):
        st.update(torch.zeros(1, 3, 32, 16, device=DEV))
    with pytest.raises(RuntimeError, match="MI355X"):
        st.update(torch.zeros(1, 3, 32, 32))


# ---- the generation pass ------------------------------------------------------------------------------------------------------
def test_evaluate_generation_spectrum_equals_the_loop_from_public_pieces():
    e, g, _, _ = build(64, "fp32")
    gen = torch.Generator().manual_seed(5)
    vl = [(torch.rand(b, 3, 64, 64, generator=gen) * 2 - 1).to(DEV) for b in (8, 8, 5)]
    zs = [torch.randn(r.shape[0], 100, generator=gen).to(DEV) for r in vl]
    nf = lambda i, b: zs[i]                                                            # noqa: E731
    keys = {"lsd_db", "hf_excess_db", "hf_share_real", "hf_share_fake"}
    base = V.evaluate_generation(g, vl, noise_fn=nf)
    got = V.evaluate_generation_spectrum(g, vl, noise_fn=nf)
    assert set(base) == {"ssim", "samples", "batches"} and set(got) == set(base) | keys
    assert all(got[k] == base[k] for k in base)
    p = S.spectrum_plan(64, 64)
    real, fake = M.SpectrumStats(p), M.SpectrumStats(p)
    g.eval()
    for i, r in enumerate(vl):
        real.update(r)
        fake.update(g.decode_eval(latent._normal_z(g, r.shape[0], zs[i]), r.shape[0]))
    want = V.spectral_distance(real, fake)
    assert all(got[k] == want[k] for k in keys) and np.isfinite([got[k] for k in keys]).all()
    # with features, KID and another bin count: the other keys are evaluate_generation's, bit for bit
    fn = V.encoder_features(e)
    kw = dict(noise_fn=nf, feature_fn=fn, kid_subsets=3, kid_subset_size=10, kid_seed=1)
    base = V.evaluate_generation(g, vl, **kw)
    got = V.evaluate_generation_spectrum(g, vl, spectrum_bins=16, window="none", **kw)
    assert set(got) == set(base) | keys and all(got[k] == base[k] for k in base)
    p = S.spectrum_plan(64, 64, 16, window="none")
    real, fake = M.SpectrumStats(p), M.SpectrumStats(p)
    for i, r in enumerate(vl):
        real.update(r)
        fake.update(g.decode_eval(latent._normal_z(g, r.shape[0], zs[i]), r.shape[0]))
    want = V.spectral_distance(real, fake)
    assert all(got[k] == want[k] for k in keys)
    with pytest.raises(RuntimeError, match="n_bins"):
        V.evaluate_generation_spectrum(g, vl, spectrum_bins=65, noise_fn=nf)


# ---- what the metric is for ---------------------------------------------------------------------------------------------------
def test_checkerboard_detection_on_the_device():
    """The condition of the CPU detection test, through SpectrumStats: +-0.02 of checkerboard on 128 smooth 64 x 64 images
    lifts the last radial bin at least 10 dB above what two independent clean sets differ by."""
    n, Sz = 128, 64
    a, b = R.smooth_images(n, Sz, 1), R.smooth_images(n, Sz, 2)
    dirty = a + R.checkerboard(Sz)[None, None]
    p = S.spectrum_plan(Sz, Sz)
    sa, sb, sd = (M.SpectrumStats(p).update(torch.from_numpy(s).to(DEV)) for s in (a, b, dirty))
    ma, mb, md = sa.mean_profile(), sb.mean_profile(), sd.mean_profile()
    lift, clean = 10 * np.log10(md[-1] / ma[-1]), abs(10 * np.log10(mb[-1] / ma[-1]))
    dc, dd = V.spectral_distance(sa, sb), V.spectral_distance(sa, sd)
    print(f"device: last-bin lift {lift:.2f} dB (clean pair {clean:.2f} dB), lsd_db {dc['lsd_db']:.2f} -> {dd['lsd_db']:.2f}, "
          f"hf_excess_db {dd['hf_excess_db']:.2f}")
    assert lift >= clean + 10.0 and dd["lsd_db"] > dc["lsd_db"] and dd["hf_excess_db"] > 0
    assert np.allclose(ma, R.profiles_fft(a)[0].mean(0), rtol=1e-9)
