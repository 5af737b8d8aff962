"""No GPU: the reference that test-time latent refinement is tested against (tests/_refine_ref.py) is itself checked against
torch -- the three kernel restatements against autograd / torch.optim.Adam, the whole loop's keep-best bookkeeping on
reference-shaped eval-mode networks at S = 16 -- then the exact-input table of the GPU test (exactness and blind spots), the
exported symbols, the host-side argument checks of the new C entry points and LatentRefiner's argument validation."""
import ctypes
import math
import os
import re
from importlib import import_module

import numpy as np
import pytest
import torch

import _refine_ref as RR
from _pairloss_ref import NAN, region_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
EINVAL, EALIGN, ENOSUP = -1, -2, -3


# ---- (a) against autograd --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act,slope", [(RR.ACT_RELU, 0.0), (RR.ACT_LRELU, 0.2), (RR.ACT_NONE, 0.0)], ids=["relu", "lrelu", "none"])
def test_bn_act_backward_eval_is_autograd_of_act_of_scale_x_plus_shift(act, slope):
    rng = np.random.default_rng(11 + act)
    rows, C = 37, 24
    x, dy = rng.standard_normal((rows, C)).astype(np.float32), rng.standard_normal((rows, C)).astype(np.float32)
    scale = (rng.standard_normal(C) + 0.2).astype(np.float32)
    shift = rng.standard_normal(C).astype(np.float32)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    z = torch.from_numpy(scale).double() * xt + torch.from_numpy(shift).double()
    y = {RR.ACT_RELU: torch.relu, RR.ACT_LRELU: lambda t: torch.nn.functional.leaky_relu(t, float(np.float32(slope))),
         RR.ACT_NONE: lambda t: t}[act](z)
    (want,) = torch.autograd.grad(y, xt, torch.from_numpy(dy).double())
    got = RR.bn_act_backward_eval(x, dy, scale, shift, act, slope)
    assert got.dtype == np.float32
    # two f32 roundings at most (dy * slope, then * scale)
    assert np.all(np.abs(got - want.numpy()) <= 2.0 ** -23 * np.abs(want.numpy()))
    got16 = RR.bn_act_backward_eval(x, dy, scale, shift, act, slope, bf16=True)
    # bf16 keeps 8 significant bits: half an ulp is 2^-8 of the value at most
    assert np.all(np.abs(got16 - want.numpy()) <= (2.0 ** -8 + 2.0 ** -22) * np.abs(want.numpy()))
    assert np.array_equal(got16, RR.bf16_round(got16))


def test_bn_act_backward_eval_at_z_zero_takes_the_negative_branch():
    x, dy = np.array([[2.0, 2.0, 1.0]], np.float32), np.array([[3.0, 3.0, 3.0]], np.float32)
    scale, shift = np.array([0.5, 0.5, 0.5], np.float32), np.array([-1.0, -0.5, -1.0], np.float32)     # z = 0, 0.5, -0.5
    assert RR.bn_act_backward_eval(x, dy, scale, shift, RR.ACT_RELU, 0.0).tolist() == [[0.0, 1.5, 0.0]]
    assert RR.bn_act_backward_eval(x, dy, scale, shift, RR.ACT_LRELU, 0.25).tolist() == [[0.375, 1.5, 0.375]]
    assert RR.bn_act_backward_eval(x, dy, scale, shift, RR.ACT_NONE, 0.0).tolist() == [[1.5, 1.5, 1.5]]


# ---- (b) against autograd, and the contract's edge cases -----------------------------------------------------------------------
def _rects(rows):
    return torch.tensor([[0.5, 0.1, rh, rw, x, y, 0, 0] for rh, rw, x, y in rows], dtype=torch.float32)


def test_masked_mse_rows_is_autograd_of_the_per_image_masked_mean():
    g = torch.Generator().manual_seed(3)
    a, b = torch.rand(4, 3, 16, 18, generator=g) * 2 - 1, torch.rand(4, 3, 16, 18, generator=g) * 2 - 1
    rects = _rects([(5, 6, 3, 4), (1, 1, 17, 15), (16, 18, 0, 0), (4, 7, 2, 9)])
    at = a.double().requires_grad_(True)
    rows = RR.masked_mean_torch(at, b.double(), rects)
    (want,) = torch.autograd.grad(0.37 * rows.sum(), at)
    loss, grad, n_valid = RR.masked_mse_rows(a, b, rects, 0.37)
    assert torch.allclose(loss, rows.detach(), rtol=1e-13, atol=0)
    assert torch.allclose(grad, want * (float(np.float32(0.37)) / 0.37), rtol=1e-12, atol=1e-18)
    assert n_valid.tolist() == [3 * (16 * 18 - 30), 3 * (16 * 18 - 1), 0, 3 * (16 * 18 - 28)]
    assert float(loss[2]) == 0.0 and not grad[2].any(), "a full-image hole: value 0, gradient 0"
    hole = region_mask(rects, *a.shape)
    assert not grad[hole].any() and (grad[~hole] != 0).all()


def test_masked_mse_rows_edge_cases_of_the_hole_rule():
    g = torch.Generator().manual_seed(4)
    a, b = torch.rand(6, 2, 8, 8, generator=g), torch.rand(6, 2, 8, 8, generator=g)
    rects = _rects([(0, 3, 1, 1), (3, 0, 1, 1), (8, 8, 5, 4), (NAN, 5, NAN, 1), (2, 2, -1, -1), (8, 8, 0, 0)])
    loss, grad, n_valid = RR.masked_mse_rows(a, b, rects)
    plain, pgrad, _ = RR.masked_mse_rows(a, b, None)
    full = 2 * 8 * 8
    #                          empty, empty, clipped to 4 x 3, NaN, clipped to 1 x 1, the whole image
    assert n_valid.tolist() == [full, full, full - 2 * 12, full, full - 2, 0]
    for i in (0, 1, 3):
        assert float(loss[i]) == float(plain[i]) and torch.equal(grad[i], pgrad[i]), i
    assert torch.allclose(plain, ((a.double() - b.double()) ** 2).reshape(6, -1).mean(1), rtol=1e-14)
    assert float(loss[5]) == 0.0


# ---- (c) against torch.optim.Adam ----------------------------------------------------------------------------------------------
def test_latent_adam_follows_torch_adam_per_row_on_the_explicit_objective():
    """Rows at DIFFERENT step counts (row 1 starts two steps late) against one torch.optim.Adam per row on
    J_i = c_i . z_i + prior_weight |z_i|^2 / (2 L): the kernel's g = dz + prior_weight z / L is its gradient."""
    B, L, ZP, pw, lr = 2, 100, 104, 0.3, 0.05
    rng = np.random.default_rng(5)
    z0 = rng.standard_normal((B, ZP)).astype(np.float32)
    z0[:, L:] = 0
    c = rng.standard_normal((3, B, ZP)).astype(np.float32) * 0.1
    ad = RR.LatentAdam(B, L, ZP)
    ad.init(z0)
    zs = [torch.from_numpy(z0[i, :L].astype(np.float64)).requires_grad_(True) for i in range(B)]
    opts = [torch.optim.Adam([z], lr=lr) for z in zs]
    for k in range(3):
        dz = c[k].copy()
        if k < 2:                                       # row 1 idles: restore its state after the call
            keep = [t[1].copy() for t in (ad.z, ad.m, ad.v)] + [int(ad.t[1])]
        loss_rows = np.array([float((c[k][i, :L].astype(np.float64) * ad.z[i].astype(np.float64)).sum()) for i in range(B)], np.float32)
        J, z_out = ad.update(dz, loss_rows, lr=lr, prior_weight=pw)
        assert not z_out[:, L:].any() and np.array_equal(z_out[:, :L], ad.z)
        if k < 2:
            ad.z[1], ad.m[1], ad.v[1], ad.t[1] = keep
        for i in range(B):
            if i == 1 and k < 2:
                continue
            opts[i].zero_grad()
            obj = (torch.from_numpy(c[k][i, :L].astype(np.float64)) * zs[i]).sum() + \
                float(np.float32(pw)) * (zs[i] ** 2).sum() / (2 * L)
            assert abs(float(J[i]) - float(obj.detach())) <= 2.0 ** -22 * max(1.0, abs(float(obj.detach()))), (k, i)
            obj.backward()
            opts[i].step()
    assert ad.t.tolist() == [3, 1]
    for i in range(B):
        # f32 state against f64: each of <= 3 steps rounds m, v, z once (2^-24 each); an Adam step is lr-sized
        assert np.abs(ad.z[i] - zs[i].detach().numpy()).max() <= 3 * (2.0 ** -23 * np.abs(ad.z[i]).max() + lr * 2.0 ** -20), i


def test_latent_adam_keep_best_is_strict_and_never_takes_a_nan():
    B, L, ZP = 3, 5, 8
    ad = RR.LatentAdam(B, L, ZP)
    z0 = np.arange(B * ZP, dtype=np.float32).reshape(B, ZP)
    ad.init(z0)
    assert np.isinf(ad.best_loss).all() and np.array_equal(ad.best_z, z0[:, :L]) and not ad.t.any()
    dz = np.ones((B, ZP), np.float32)
    ad.update(dz, np.array([1.0, 2.0, NAN], np.float32))
    assert ad.best_loss.tolist()[:2] == [1.0, 2.0] and np.isinf(ad.best_loss[2])
    first = ad.best_z.copy()
    assert np.array_equal(first, z0[:, :L]), "the best z is the one that was evaluated, not the updated one"
    ad.update(dz, np.array([1.0, 1.5, NAN], np.float32))        # a tie, an improvement, a NaN again
    assert ad.best_loss.tolist()[:2] == [1.0, 1.5] and np.isinf(ad.best_loss[2])
    assert np.array_equal(ad.best_z[0], first[0]) and not np.array_equal(ad.best_z[1], first[1]) and np.array_equal(ad.best_z[2], first[2])
    before = (ad.z.copy(), ad.t.copy())
    ad.track(np.array([0.5, 9.0, 0.25], np.float32))            # TRACK: bookkeeping only
    assert np.array_equal(ad.z, before[0]) and np.array_equal(ad.t, before[1]) and ad.best_loss.tolist() == [0.5, 1.5, 0.25]
    assert np.array_equal(ad.best_z[0], ad.z[0]) and np.array_equal(ad.best_z[2], ad.z[2])
    # the adversarial term: nn.BCELoss' clamp
    J = RR.LatentAdam(2, L, ZP).objective(np.zeros(2, np.float32), np.array([0.5, 0.0], np.float32), 0.1, 0.0)
    assert abs(float(J[0]) - 0.1 * math.log(2.0)) < 1e-8 and abs(float(J[1]) - 10.0) < 1e-6


# ---- the whole loop ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case():
    nets = RR.Nets()
    return nets, RR.make_case(nets)


@pytest.mark.parametrize("alpha_adv", [0.0, 0.1])
def test_loop_keeps_the_best_iterate_and_the_chosen_seed_descends(case, alpha_adv):
    nets, (noisy, rects, z_star, z0) = case
    out = RR.refine_loop(nets, noisy, rects, z0, 5, alpha_adv=alpha_adv, prior_weight=RR.CASE_PRIOR)
    obj = out["objectives"]                                     # [6, B]
    assert obj.shape == (6, 4) and torch.isfinite(obj).all()
    assert torch.equal(out["best"], obj.min(0).values) and (out["best"] <= obj[0]).all()
    # z equals the argmin of the recorded objectives: re-run, keeping every iterate
    iterates = [RR.refine_loop(nets, noisy, rects, z0, k, alpha_adv=alpha_adv, prior_weight=RR.CASE_PRIOR)["z"] for k in range(6)]
    arg = obj.argmin(0)
    for i in range(4):
        assert torch.equal(out["best_z"][i], iterates[int(arg[i])][i]), i
    # what CASE_SEED was chosen for (the GPU test relies on it): every image's objective ends strictly lower, and no gradient
    # component is within two orders of magnitude of Adam's eps, where g / (|g| + eps) stops being a sign
    assert (obj[-1] < obj[0]).all() and (out["best"] < obj[0]).all()
    assert float(out["grads"].abs().min()) > 1e2 * 1e-8


def test_loop_targets_have_a_painted_rectangle_and_rows_do_not_mix(case):
    nets, (noisy, rects, z_star, z0) = case
    hole = region_mask(rects, *noisy.shape)
    assert hole.any(1).any(1).any(1).all() and (noisy[hole] == 1.0).all()
    with torch.no_grad():
        assert torch.equal(noisy[~hole], nets.decode(z_star.double()).float()[~hole])
    a = RR.refine_loop(nets, noisy, rects, z0, 2, alpha_adv=0.1)
    perm = [0, 3, 2, 1]
    b = RR.refine_loop(nets, noisy[perm], rects[perm], z0[perm], 2, alpha_adv=0.1)
    assert torch.allclose(a["z"][0], b["z"][0], rtol=0, atol=1e-14)


# ---- the exact-input table of tests/test_gpu_refine.py -----------------------------------------------------------------------
EXACT_SHAPES = [(r, c) for r in (1, 37, 300) for c in (8, 24, 264)]


def _fits_bf16(t):
    return np.array_equal(RR.bf16_round(t), t)


@pytest.mark.parametrize("rows,C", EXACT_SHAPES)
def test_exact_cases_are_exact_and_have_no_blind_spot(rows, C):
    x, dy, scale, shift = RR.exact_case(100 + rows + C, rows, C)
    assert all(_fits_bf16(t) for t in (x, dy)) and (x != 0).all() and (dy != 0).all()
    z = scale.astype(np.float64) * x + shift
    assert (z[0, :4] == 0).all() and (rows == 1 or ((z > 0).any() and (z < 0).any()))
    assert (scale[1:] != scale[:-1]).all() and scale[0] != scale[-1] and (np.abs(shift)[1:] != np.abs(shift)[:-1]).any()
    for act in (RR.ACT_NONE, RR.ACT_RELU, RR.ACT_LRELU):
        base = RR.bn_act_backward_eval(x, dy, scale, shift, act, RR.EXACT_SLOPE)
        # exact: the f64 value of the expression is the f32 result, and bf16 holds it
        dz = dy.astype(np.float64) if act == RR.ACT_NONE else np.where(z > 0, dy, dy * (RR.EXACT_SLOPE if act == RR.ACT_LRELU else 0.0))
        assert np.array_equal(base.astype(np.float64), dz * scale) and _fits_bf16(base)
        assert np.array_equal(RR.bn_act_backward_eval(x, dy, scale, shift, act, RR.EXACT_SLOPE, bf16=True), base)
        differs = lambda other: not np.array_equal(other, base)                                    # noqa: E731
        assert differs(RR.bn_act_backward_eval(x, dy, np.roll(scale, 1), shift, act, RR.EXACT_SLOPE)), "scale of channel c - 1"
        assert differs(RR.bn_act_backward_eval(x, dy, np.roll(scale, -1), shift, act, RR.EXACT_SLOPE)), "scale of channel c + 1"
        assert differs(RR.bn_act_backward_eval(x, dy, np.ones_like(scale), shift, act, RR.EXACT_SLOPE)), "the factor scale dropped"
        if act != RR.ACT_NONE:
            flipped = np.where(z[0, :4] == 0, dy[0, :4] * scale[:4], base[0, :4])      # z >= 0 taken as positive
            assert not np.array_equal(flipped, base[0, :4]), "z == 0 on the positive branch"
            if rows > 1:
                assert differs(RR.bn_act_backward_eval(x, dy, scale, np.zeros_like(shift), act, RR.EXACT_SLOPE)), "shift dropped"
                assert differs(RR.bn_act_backward_eval(x, dy, scale, np.roll(shift, 1), act, RR.EXACT_SLOPE)), "shift of channel c - 1"
                assert differs(RR.bn_act_backward_eval(x[::-1], dy, scale, shift, act, RR.EXACT_SLOPE)), "x of another row"


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
NEW = ("vg_bn_act_backward_eval", "vg_masked_mse_rows", "vg_masked_mse_rows_ws_doubles", "vg_latent_adam")


def test_new_symbols_are_declared_bound_and_exported_with_the_abi_still_at_31():
    L = import_module(PKG + "._lib")
    lib = L.load()
    src = open(os.path.join(ROOT, "include", "vaegan_hip.h")).read()
    assert int(re.search(r"#define\s+VG_ABI_VERSION\s+(\d+)", src).group(1)) == L.ABI_VERSION == 31
    assert lib.vg_abi_version() == 31
    for name in NEW:
        assert name in L.SIGNATURES and re.search(r"\b%s\s*\(" % name, src), name
        assert getattr(lib, name) is not None
    for name, val in (("VG_LATENT_INIT", 0), ("VG_LATENT_UPDATE", 1), ("VG_LATENT_TRACK", 2)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, src).group(1)) == getattr(L, name) == val
    ops = import_module(PKG + ".ops")
    assert all(callable(getattr(ops, n)) for n in ("bn_act_backward_eval", "masked_mse_rows", "latent_adam", "latent_state"))
    assert "refine.hip" in open(os.path.join(ROOT, PKG, "csrc", "Makefile")).read()
    assert not any(k.startswith("VG_BN_PLAN") and "EVAL" in k for k in re.findall(r"#define\s+(\w+)", src))


def test_c_abi_rejects_bad_arguments_of_the_new_entry_points_on_host():
    """Validation happens before any launch (pattern: test_host_cpu.test_c_abi_rejects_bad_arguments_on_host)."""
    lib = import_module(PKG + "._lib").load()
    buf, odd8, odd4 = ctypes.c_void_p(4096), ctypes.c_void_p(4104), ctypes.c_void_p(4100)    # never dereferenced
    e = lib.vg_bn_act_backward_eval
    ok = dict(x=buf, dy=buf, dx=buf, scale=buf, shift=buf, rows=37, C=24, act=1, slope=0.0, dtype=0, stream=None)

    def ev(**kw):
        return e(*dict(ok, **kw).values())

    for name in ("x", "dy", "dx", "scale", "shift"):
        assert ev(**{name: None}) == EINVAL, name
    for kw in (dict(rows=0), dict(rows=-1), dict(C=0), dict(act=3), dict(act=-1), dict(act=7)):
        assert ev(**kw) == EINVAL, kw
    assert ev(dtype=2) == ENOSUP and ev(dtype=-1) == ENOSUP
    assert ev(C=22) == EALIGN
    for name in ("x", "dy", "dx"):
        assert ev(**{name: odd8}) == EALIGN, name                        # f32: 16-byte vectors
        assert ev(**{name: odd4, "dtype": 1}) == EALIGN, name            # bf16: 8 bytes at least
    assert ev(scale=odd8) == EALIGN and ev(shift=odd8, dtype=1) == EALIGN

    q, m = lib.vg_masked_mse_rows_ws_doubles, lib.vg_masked_mse_rows
    for bad in ((0, 3, 16, 16), (2, 0, 16, 16), (2, 3, 0, 16), (2, 3, 16, 0), (65536, 3, 16, 16), (2, 1 << 11, 1 << 10, 1 << 10)):
        assert q(*bad) == EINVAL, bad
    n = q(3, 3, 16, 16)
    assert n == 3 * 3 and q(128, 3, 64, 64) == 128 * 16
    ok = dict(a=buf, b=buf, rects=buf, B=3, C=3, H=16, W=16, gscale=1.0, loss=buf, da=buf, ws=buf, nws=n, stream=None)

    def mm(**kw):
        return m(*dict(ok, **kw).values())

    assert mm(a=None) == EINVAL and mm(b=None) == EINVAL and mm(ws=None) == EINVAL and mm(nws=n - 1) == EINVAL
    assert mm(loss=None, da=None) == EINVAL
    assert mm(gscale=float("inf")) == EINVAL and mm(gscale=float("nan")) == EINVAL
    for kw in (dict(B=0), dict(C=0), dict(H=0), dict(W=-1), dict(B=65536)):
        assert mm(**kw) == EINVAL, kw
    assert mm(rects=odd4) == EALIGN and mm(ws=odd4) == EALIGN and mm(a=ctypes.c_void_p(4097)) == EALIGN

    f = lib.vg_latent_adam
    ok = dict(z=buf, m=buf, v=buf, t=buf, best=buf, best_z=buf, dz=buf, loss=buf, p=None, z_in=buf, z_out=buf, obj=None, B=4,
              L=100, ZP=104, lr=0.05, b1=0.9, b2=0.999, eps=1e-8, adv=0.0, prior=0.0, mode=1, dtype=0, stream=None)

    def la(**kw):
        return f(*dict(ok, **kw).values())

    for mode in (-1, 3):
        assert la(mode=mode) == EINVAL
    for kw in (dict(B=0), dict(L=0), dict(ZP=96), dict(B=-2)):
        assert la(**kw) == EINVAL, kw
    for name in ("z", "best", "best_z"):
        for mode in (0, 1, 2):
            assert la(**{name: None, "mode": mode}) == EINVAL, (name, mode)
    for name in ("m", "v", "t", "z_in"):
        assert la(**{name: None, "mode": 0}) == EINVAL, name
    for name in ("m", "v", "t", "dz", "z_out", "loss"):
        assert la(**{name: None, "mode": 1}) == EINVAL, name
    assert la(loss=None, mode=2) == EINVAL
    for kw in (dict(lr=-1.0), dict(lr=float("nan")), dict(eps=-1e-8), dict(b1=1.0), dict(b1=-0.1), dict(b2=1.0), dict(b2=float("nan")),
               dict(adv=-0.1), dict(adv=float("inf")), dict(prior=-1.0), dict(prior=float("nan"))):
        assert la(**kw) == EINVAL, kw
    assert la(dtype=2) == ENOSUP
    assert la(ZP=102) == EALIGN
    assert la(dz=ctypes.c_void_p(4098)) == EALIGN and la(z_out=ctypes.c_void_p(4097), dtype=1) == EALIGN


# ---- LatentRefiner's arguments -----------------------------------------------------------------------------------------------
def test_latent_refiner_argument_validation_never_reaches_the_device():
    V = import_module("vaegan_amd")
    e, g, d = V.Encoder([3, 64, 64], 100), V.Generator(nz=100, img_size=64), V.Discriminator(img_size=64)
    r = V.LatentRefiner(e, g, d, alpha_adv=0.1)
    assert (r.steps, r.lr, r.betas, r.eps, r.prior_weight, r.keep_best, r.graphed) == (50, 0.05, (0.9, 0.999), 1e-8, 0.0, True, True)
    assert V.LatentRefiner(e, g).D is None and V.LatentRefiner(None, g).E is None
    for kw, match in ((dict(steps=-1), "steps"), (dict(steps=2.5), "steps"), (dict(steps=True), "steps"),
                      (dict(lr=-0.1), "lr must be finite and >= 0"), (dict(lr=float("nan")), "lr"), (dict(lr="fast"), "lr"),
                      (dict(betas=(0.9,)), "betas"), (dict(betas=(0.9, 1.0)), "betas"), (dict(betas=0.9), "betas"),
                      (dict(eps=-1e-8), "eps must be finite and >= 0"),
                      (dict(alpha_adv=-0.1), "alpha_adv must be finite and >= 0"), (dict(alpha_adv=float("inf")), "alpha_adv"),
                      (dict(prior_weight=-1.0), "prior_weight must be finite and >= 0"),
                      (dict(keep_best=1), "keep_best must be True or False"), (dict(graphed=None), "graphed must be True or False")):
        with pytest.raises(ValueError, match=match):
            V.LatentRefiner(e, g, d, **kw)
    with pytest.raises(ValueError, match="needs a discriminator"):
        V.LatentRefiner(e, g, alpha_adv=0.1)
    with pytest.raises(ValueError, match="share one engine dtype"):
        V.LatentRefiner(e, V.Generator(nz=100, img_size=64, dtype="bf16"))
    with pytest.raises(ValueError, match="Encoder's latent"):
        V.LatentRefiner(e, V.Generator(nz=64, img_size=64))
    with pytest.raises(ValueError, match="Generator's image shape"):
        V.LatentRefiner(e, g, V.Discriminator(img_size=32), alpha_adv=0.1)
    with pytest.raises(TypeError):                                      # keyword-only
        V.LatentRefiner(e, g, d, 5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        r.refine(torch.zeros(2, 3, 64, 64))
    with pytest.raises(ValueError, match="refine must be"):
        V.paired_test_epoch(e, g, [], refine=5)
    with pytest.raises(ValueError, match="other networks"):
        V.paired_test_epoch(e, V.Generator(nz=100, img_size=64), [], refine=r)
    with pytest.raises(RuntimeError, match="want_rects"):
        V.paired_test_epoch(e, g, [], refine=r)
    eng = g._engine
    with pytest.raises(RuntimeError, match="eval-mode network is not supported"):
        eng.backward(([], 2, False), None, True, None, param_grads=True)
    with pytest.raises(ValueError, match="eval-mode backward"):
        eng.backward(([], 2, False), None, True, None, param_grads=False, weight_grad_groups=2)
    with pytest.raises(ValueError, match="eval-mode backward"):
        eng.backward(([], 2, False), None, True, None, param_grads=False, feat=(1, None, 1.0, None))
