"""No GPU: the references that training on degraded pairs is tested against (tests/_pairloss_ref.py) are themselves checked
-- the region-weighted gradient against torch.autograd, the masks against the contract's edge cases, ref_step / ref_vae_step
against the oracles they extend -- and the exported symbols, the host-side argument checks of the C entry points and of
the trainers / the loader against the built library and the package."""
import ctypes
import os
import re
from importlib import import_module

import pytest
import torch

import _pairloss_ref as PR
import _pointwise_ref as P
import siblings_ref as SIB
import vaegan_ref as R
from _inputs import make_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
SHAPES = [(1, 1, 4, 4), (3, 3, 5, 7), (2, 1, 12, 20), (2, 3, 16, 16), (5, 3, 64, 64)]


def _ab(shape, seed=0):
    g = P.gen(seed + sum(shape))
    return torch.rand(shape, generator=g) * 2 - 1, torch.rand(shape, generator=g) * 2 - 1


@pytest.mark.parametrize("w_hole,gscale", [(1.0, 1.0), (6.0, 0.37), (0.0, 1.0), (0.25, 0.37)])
@pytest.mark.parametrize("shape", SHAPES)
def test_region_mse_grad_equals_autograd_of_the_masked_expression(shape, w_hole, gscale):
    B, C, H, W = shape
    a, b = _ab(shape)
    for shift in range(0, 8, B):
        rects = PR.offset_rects(B, H, W, shift)
        m = PR.region_mask(rects, *shape).double()
        x = a.double().requires_grad_(True)
        loss = ((m * P.f32(w_hole) + (1 - m)) * (x - b.double()) ** 2).sum() / x.numel()
        (P.f32(gscale) * loss).backward()
        g = PR.region_mse_grad(a, b, rects, w_hole, gscale)
        scale = float(x.grad.abs().max())
        assert float((g - x.grad).abs().max()) <= 1e-12 * max(scale, 1e-300)
        got = PR.region_mse(a, b, rects, w_hole)
        assert abs(got[0] - float(loss.detach())) <= 1e-12 * max(float(loss.detach()), 1e-300)
        assert got[4] + got[5] == a.numel() and got[4] == int(m.sum())
        l_w, hole = PR.weighted_mse(a.double(), b.double(), rects, P.f32(w_hole))
        assert abs(float(l_w) - got[0]) <= 1e-12 * max(got[0], 1e-300) and abs(float(hole) - got[1]) <= 1e-12 * max(got[1], 1e-300)


@pytest.mark.parametrize("shape", SHAPES)
def test_w_hole_one_and_no_rects_reduce_to_the_plain_mse(shape):
    B, C, H, W = shape
    a, b = _ab(shape, 1)
    ref = float(P.mse(a, b))
    for rects in (None, PR.cycle_rects(B, H, W)):
        got = PR.region_mse(a, b, rects, 1.0)
        assert abs(got[0] - ref) <= 1e-14 * ref
        assert torch.allclose(PR.region_mse_grad(a, b, rects, 1.0, 0.37), P.mse_grad(a, b, 0.37), rtol=1e-14, atol=0)
    none = PR.region_mse(a, b, None, 6.0)
    assert none[1] == 0.0 and none[2] == 0.0 and none[4] == 0 and none[5] == a.numel() and abs(none[0] - ref) <= 1e-14 * ref


def test_masks_of_the_contracts_edge_cases():
    B, C, H, W = 8, 2, 12, 20
    m = PR.region_mask(PR.cycle_rects(B, H, W), B, C, H, W)
    assert m.shape == (B, C, H, W) and torch.equal(m[:, 0], m[:, 1])            # every channel
    counts = [int(m[i, 0].sum()) for i in range(B)]
    assert counts[0] == 0 and counts[1] == 0                                     # empty by height, by width
    assert counts[2] == H * W and bool(m[2].all())                               # the full image
    assert counts[3] == 1 and bool(m[3, 0, 0, 0])
    assert counts[4] == 1 and bool(m[4, 0, H - 1, W - 1])
    assert counts[5] == 4 * 6 and bool(m[5, 0, 1:5, 5:11].all()) and not bool(m[5, 0, 1, 4]) and not bool(m[5, 0, 1, 11])
    assert counts[6] == (H - H // 2) * (W - (W // 2 + 1)) and bool(m[6, 0, H // 2:, W // 2 + 1:].all())   # clipped
    assert counts[7] == 0                                                        # a NaN row: no hole
    for bad in ([1, 1, 4, 4, PR.NAN, 2], [1, 1, PR.NAN, 4, 2, 2], [1, 1, 4, PR.NAN, 2, 2], [1, 1, 4, 4, 2, PR.NAN]):
        r = torch.tensor([bad + [0, 0]], dtype=torch.float32)
        assert int(PR.region_mask(r, 1, 1, H, W).sum()) == 0
    neg = torch.tensor([[0, 0, 6, 6, -2, -3, 0, 0]], dtype=torch.float32)        # reaching past the left and top edges
    assert int(PR.region_mask(neg, 1, 1, H, W).sum()) == 3 * 4
    assert int(PR.region_mask(None, 2, 3, 4, 4).sum()) == 0
    # make_noisy: outside the holes the input is the clean image + noise, inside it is not
    clean = torch.zeros(4, 3, 64, 64)
    rects = PR.hand_rects(4)
    noisy = PR.make_noisy(clean, rects, 3, sigma=0.0)
    mm = PR.region_mask(rects, 4, 3, 64, 64)
    assert float(noisy[~mm].abs().max()) == 0.0 and float(noisy[mm].abs().mean()) > 0.3
    assert [int(mm[i, 0].sum()) for i in range(4)] == [rh * rw for rh, rw, _, _ in PR.HAND_RECTS]


def _same_state(a, b):
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_ref_step_with_nothing_to_pair_is_the_oracle_step_bit_for_bit():
    S, B = 64, 4
    a, b, c = (R.RefVAEGAN(img_size=S, seed=42) for _ in range(3))
    real, ez, er, ec = make_inputs(B, S, 7000 + S)                    # the inputs of oracle_steps_S64_B4
    la = a.train_step(real, ez, er, ec, 60)
    lb = PR.ref_step(b, real, real.clone(), ez, er, ec, 60, hole_weight=1.0)
    assert la == lb
    lc = PR.ref_step(c, real, real.clone(), ez, er, ec, 60, rects=PR.hand_rects(B), hole_weight=1.0)
    assert la == lc
    for x in (b, c):
        for sa, sb in ((a.E, x.E), (a.G, x.G), (a.D, x.D)):
            _same_state(sa, sb)
        for oa, ob in ((a.opt_E, x.opt_E), (a.opt_G, x.opt_G), (a.opt_D, x.opt_D)):
            assert oa.t == ob.t
            for p, q in zip(oa.exp_avg + oa.exp_avg_sq, ob.exp_avg + ob.exp_avg_sq):
                assert torch.equal(p, q)


def test_ref_step_with_the_weight_on_moves_what_it_should():
    S, B = 64, 4
    a, b = R.RefVAEGAN(img_size=S, seed=42), R.RefVAEGAN(img_size=S, seed=42)
    real, ez, er, ec = make_inputs(B, S, 7000 + S)
    rects = PR.hand_rects(B)
    noisy = PR.make_noisy(real, rects, 11)
    la = PR.ref_step(a, real, noisy, ez, er, ec, 60, rects=rects, hole_weight=1.0)
    lb = PR.ref_step(b, real, noisy, ez, er, ec, 60, rects=rects, hole_weight=6.0)
    assert "hole_mse" not in la and lb["hole_mse"] > 0
    # L_w = mse + (w - 1) * hole_fraction * hole_mse
    frac = sum(rh * rw for rh, rw, _, _ in PR.HAND_RECTS) / (B * S * S)
    assert abs(lb["recon_loss"] - (la["recon_loss"] + 5.0 * frac * lb["hole_mse"])) <= 1e-5 * lb["recon_loss"]
    for k in ("kl_loss", "d_loss_1", "d_loss_2", "g_loss_adv"):
        assert la[k] == lb[k]
    _same_state(a.D, b.D)                                             # its two updates precede the term
    assert not torch.equal(a.opt_G.exp_avg[0], b.opt_G.exp_avg[0]) and not torch.equal(a.opt_E.exp_avg[0], b.opt_E.exp_avg[0])


def test_ref_vae_step_with_nothing_to_pair_is_the_sibling_oracle_bit_for_bit():
    S, B = 64, 2
    g = P.gen(8100)
    img = torch.rand(B, 3, S, S, generator=g) * 2 - 1
    eps_img, eps_z = torch.randn(B, 3, S, S, generator=g), torch.randn(B, 100, generator=g)
    a, b, c = (SIB.RefVAE(img_size=S, seed=42) for _ in range(3))
    la = a.train_step(img, eps_img, eps_z, 25)
    noisy = torch.clamp(img + eps_img * 0.5, -1.0, 1.0)
    lb = PR.ref_vae_step(b, img, noisy, eps_z, 25)
    assert la == lb
    _same_state(a.E, b.E), _same_state(a.G, b.G)
    lc = PR.ref_vae_step(c, img, noisy, eps_z, 25, rects=PR.hand_rects(B), hole_weight=6.0)
    assert lc["kl_loss"] == la["kl_loss"] and lc["recon_loss"] > la["recon_loss"] and lc["hole_mse"] > 0
    assert not torch.equal(a.opt.exp_avg[0], c.opt.exp_avg[0])


def test_isolation_input_keeps_every_activation_away_from_its_kink():
    """The degraded input of tests/test_gpu_pairloss.test_weighted_gradient_path_in_isolation_vs_fp64_ref_step is chosen from
    the fp64 oracle alone: on it the CPU fp32 forward takes every ReLU / LeakyReLU branch the fp64 one takes."""
    import _ssimloss_ref as SR
    o64 = R.RefVAEGAN(img_size=64, seed=42, lr=0.0).double_()
    o32 = R.RefVAEGAN(img_size=64, seed=42, lr=0.0)
    real, ez, _, _ = make_inputs(4, 64, SR.ISO_SEED)
    rects = PR.hand_rects(4)
    margins = [SR.activation_margin(o64, PR.make_noisy(real, rects, s), ez)[0] for s in range(PR.NOISY_SEED, PR.ISO_NOISY_SEED + 1)]
    assert [m >= 2e-6 for m in margins] == [False] * (len(margins) - 1) + [True]
    noisy = PR.make_noisy(real, rects, PR.ISO_NOISY_SEED)
    p64, p32 = SR.activation_margin(o64, noisy, ez)[1], SR.activation_margin(o32, noisy, ez)[1]
    assert sum(int(((a.double() > 0) != (b > 0)).sum()) for a, b in zip(p32, p64)) == 0


def test_ref_paired_regions_accumulates_over_batches_and_survives_empty_regions():
    a, b = _ab((2, 3, 16, 16), 2)
    rects = PR.cycle_rects(8, 16, 16)[2:4]                            # the full image, 1 x 1
    one = PR.ref_paired_regions([(a, b, b.clone(), rects)])
    assert one["hole_fraction"] == (256 + 1) / 512 and one["mse_hole_noisy"] == 0.0 and one["psnr_hole_noisy"] == float("inf")
    two = PR.ref_paired_regions([(a[:1], b[:1], b[:1], rects[:1]), (a[1:], b[1:], b[1:], rects[1:])])
    for k in one:
        assert abs(one[k] - two[k]) <= 1e-12 * max(abs(one[k]), 1e-300) or one[k] == two[k]
    none = PR.ref_paired_regions([(a, b, b, None)])
    assert none["hole_fraction"] == 0.0 and none["mse_hole"] == 0.0 and none["psnr_hole"] == float("inf")
    assert abs(none["mse_valid"] - float(P.mse(a, b))) <= 1e-14


def test_new_symbols_are_exported_and_the_abi_version_moved():
    L = import_module(PKG + "._lib")
    lib = L.load()
    src = open(os.path.join(ROOT, "include", "vaegan_hip.h")).read()
    assert int(re.search(r"#define\s+VG_ABI_VERSION\s+(\d+)", src).group(1)) == L.ABI_VERSION >= 18
    assert lib.vg_abi_version() == L.ABI_VERSION
    for name in ("vg_region_mse_forward_backward", "vg_region_mse_ws_doubles"):
        assert name in L.SIGNATURES and name in src
        assert getattr(lib, name) is not None
    ops = import_module(PKG + ".ops")
    assert callable(ops.region_mse_forward_backward)


def test_workspace_query():
    lib = import_module(PKG + "._lib").load()
    q = lib.vg_region_mse_ws_doubles
    # three f64 partials (S_hole, S_valid, n_hole) per workgroup; sized for the one-element-per-lane path (256 elements per
    # workgroup), which the 16-byte path never exceeds; at most 1024 workgroups
    assert q(1, 1, 4, 4) == 3 and q(5, 3, 64, 64) == 3 * 240 and q(128, 3, 64, 64) == 3 * 1024 and q(3, 3, 5, 7) == 6
    for bad in ((0, 1, 4, 4), (1, 0, 4, 4), (1, 1, 0, 4), (1, 1, 4, 0), (-1, 3, 64, 64)):
        assert q(*bad) <= 0, bad


def test_c_abi_rejects_bad_region_mse_arguments_on_host():
    """Validation happens before any launch (pattern: test_host_cpu.test_c_abi_rejects_bad_arguments_on_host)."""
    lib = import_module(PKG + "._lib").load()
    f = lib.vg_region_mse_forward_backward
    buf = ctypes.c_void_p(4096)                                       # never dereferenced: validation comes first
    EINVAL = -1
    n = lib.vg_region_mse_ws_doubles(2, 3, 16, 16)
    #          a    b    rects B  C  H   W   w    g    loss hole d_a  stats ws   cap stream
    assert f(None, buf, buf, 2, 3, 16, 16, 6.0, 1.0, buf, buf, buf, buf, buf, n, None) == EINVAL        # a NULL
    assert f(buf, None, buf, 2, 3, 16, 16, 6.0, 1.0, buf, buf, buf, buf, buf, n, None) == EINVAL        # b NULL
    for bad in ((0, 3, 16, 16), (2, 0, 16, 16), (2, 3, 0, 16), (2, 3, 16, 0), (-2, 3, 16, 16)):
        assert f(buf, buf, buf, *bad, 6.0, 1.0, buf, buf, buf, buf, buf, n, None) == EINVAL, bad
    for w in (-1.0, float("inf"), float("nan"), -0.5):
        assert f(buf, buf, buf, 2, 3, 16, 16, w, 1.0, buf, buf, buf, buf, buf, n, None) == EINVAL, w
    assert f(buf, buf, buf, 2, 3, 16, 16, 6.0, 1.0, buf, buf, buf, buf, None, n, None) == EINVAL        # no workspace
    assert f(buf, buf, buf, 2, 3, 16, 16, 6.0, 1.0, buf, buf, buf, buf, buf, n - 1, None) == EINVAL     # one double short
    assert f(buf, buf, buf, 2, 3, 16, 16, 6.0, 1.0, buf, buf, buf, buf, buf, 0, None) == EINVAL
    assert f(buf, buf, buf, 2, 3, 16, 16, 6.0, 1.0, None, None, None, None, buf, n, None) == EINVAL     # every output NULL
    assert f(buf, buf, ctypes.c_void_p(4100), 2, 3, 16, 16, 6.0, 1.0, buf, buf, buf, buf, buf, n, None) == -2   # VG_EALIGN: rects


def _nets(S=64):
    V = import_module("vaegan_amd")
    return V, V.Encoder([3, S, S], 100), V.Generator(nz=100, img_size=S), V.Discriminator(img_size=S)


def test_host_argument_checks_of_the_trainers_never_reach_the_device():
    V, e, g, d = _nets()
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            V.VAEGANTrainer(e, g, d, None, None, None, hole_weight=bad)
        with pytest.raises(ValueError):
            V.VAETrainer(e, g, None, hole_weight=bad)
    tr = V.VAEGANTrainer(e, g, d, None, None, None, hole_weight=6.0)
    assert tr.hole_weight == 6.0 and V.VAEGANTrainer(e, g, d, None, None, None).hole_weight == 1.0
    x = torch.zeros(2, 3, 64, 64)
    rects, nhwc = torch.zeros(2, 8), torch.zeros(2, 64, 64, 4)
    with pytest.raises(ValueError):
        tr.train_step(x, 60, rects=rects)                             # rects without noisy
    with pytest.raises(ValueError):
        tr.train_step(x, 60, noisy_nhwc=nhwc)                         # noisy_nhwc without noisy
    with pytest.raises(ValueError):
        tr.train_step_graphed(x, 60, rects=rects)
    with pytest.raises(ValueError):
        tr.train_step_graphed(x, 60, noisy=x, noisy_nhwc=nhwc)        # eager-only
    vt = V.VAETrainer(e, g, None, hole_weight=6.0)
    with pytest.raises(ValueError):
        vt.train_step(x, rects=rects)
    with pytest.raises(ValueError):
        vt.step_graphed(x, rects=rects)


class _FakeSet:
    """Stands in for ResidentImages where only the host-side logic runs (tests/test_degrade_cpu.py)."""
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def test_host_argument_checks_of_the_loader_and_the_wrapper():
    data = import_module(PKG + ".data")
    ops = import_module(PKG + ".ops")
    denoise = import_module(PKG + ".denoise")
    plain = data.DeviceLoader(_FakeSet(8), torch.arange(8), 4)
    clean_only = data.DeviceLoader(_FakeSet(8), torch.arange(8), 4, degrade=data.Degrade(None, normalize=False))
    for loader in (plain, clean_only):
        with pytest.raises(RuntimeError):
            loader.want_rects(True)                                   # only degraded loaders know rectangles
        with pytest.raises(RuntimeError):
            loader.bind_noisy(torch.zeros(4, 3, 8, 8))
        loader.want_rects(False), loader.bind_noisy(None)             # turning off is always fine
        assert loader.last_rects is None
    deg = data.DeviceLoader(_FakeSet(8), torch.arange(8), 4, degrade=data.Degrade(0.25))
    deg.want_rects(True)
    assert deg._rects and deg.last_rects is None
    deg.want_rects(False)
    assert not deg._rects
    with pytest.raises(RuntimeError, match="regions=True"):
        denoise.paired_test_epoch(None, None, [(None, None)], regions=True)
    with pytest.raises(RuntimeError, match="regions=True"):
        denoise.paired_test_epoch(None, None, plain, regions=True)
    a = torch.zeros(2, 3, 8, 8)
    with pytest.raises(RuntimeError):
        ops.region_mse_forward_backward(a, a, None, 1.0, 1.0, loss=torch.zeros(1))      # host tensors: no CPU path
