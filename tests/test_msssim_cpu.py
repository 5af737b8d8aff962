"""No GPU: the references the multi-scale SSIM loss is tested against (tests/_msssim_ref.py) are themselves checked -- the
autograd restatement against a second, independent formulation (explicit tap-by-tap derivative maps, the pooling adjoint
written as repeat_interleave / 4 with zero fill, the per-image coefficients k of the contract), the single-scale case
against the SSIM map, the pooling adjoint identity, ref_step / ref_vae_step against the steps they extend -- and the
default-scale rule, the exported symbols, the workspace query and every host-side argument check of the two entry points
against the built library, the keyword validation of the Python layers, and the conditions of the input table the GPU
tests (tests/test_gpu_msssim.py) rely on."""
import ctypes
import math
import os
from importlib import import_module

import pytest
import torch
import torch.nn.functional as F

import _msssim_ref as MR
import _pointwise_ref as P
import _ssimloss_ref as SR
import siblings_ref as SIB
import vaegan_ref as R
from _inputs import make_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
EINVAL = -1
torch.set_num_threads(min(16, os.cpu_count() or 1))


# ======================================================================================================================
# The restatement against independent formulations
# ======================================================================================================================
@pytest.mark.parametrize("kind", P.SSIM_KINDS)
@pytest.mark.parametrize("shape", [(1, 1, 11, 11), (2, 3, 12, 17), (2, 3, 64, 64)])
def test_single_scale_with_weight_one_is_one_minus_the_clamped_mean_ssim(kind, shape):
    a, b = P.ssim_inputs(kind, *shape)
    want = 1.0 - torch.relu(P.ssim_map(a, b).mean(dim=(1, 2, 3))).mean()
    got = MR.msssim_loss(a, b, (1.0,))
    assert abs(float(got) - float(want)) <= 1e-14
    if kind not in ("negated",) and bool((P.ssim_map(a, b).mean(dim=(1, 2, 3)) > 0).all()):
        assert abs(float(got) - float(SR.ssim_loss(a, b))) <= 1e-14      # no image on the clamp: the SSIM loss itself


def _pool(x):
    """2 x 2 mean, stride 2, trailing odd row / column dropped -- by reshape, not avg_pool2d."""
    B, C, H, W = x.shape
    h, w = H // 2, W // 2
    return x[..., :2 * h, :2 * w].reshape(B, C, h, 2, w, 2).mean(dim=(3, 5))


def _pool_t(y, H, W):
    """The adjoint of _pool onto an H x W plane: every coarse value / 4 to its four sources, zero elsewhere."""
    out = torch.zeros(y.shape[:2] + (H, W), dtype=y.dtype)
    up = y.repeat_interleave(2, -2).repeat_interleave(2, -1) / 4
    out[..., :up.shape[-2], :up.shape[-1]] = up
    return out


def _level_closed_form(a, b, cs_only):
    """-> (sum of the level's map per image [B], d(that sum) / d a [B,C,H,W]): the contract's closed form, tap by tap, f64."""
    u, v = (a + 1) * 0.5, (b + 1) * 0.5
    g = P.gauss11()
    H, W = u.shape[-2:]
    IH, IW = H - 10, W - 10
    z = torch.zeros(u.shape[:2] + (IH, IW), dtype=torch.float64)
    mu, mv, suu, svv, suv = z.clone(), z.clone(), z.clone(), z.clone(), z.clone()
    for dy in range(11):
        for dx in range(11):
            w = g[dy] * g[dx]
            pu, pv = u[..., dy:dy + IH, dx:dx + IW], v[..., dy:dy + IH, dx:dx + IW]
            mu += w * pu
            mv += w * pv
            suu += w * pu * pu
            svv += w * pv * pv
            suv += w * pu * pv
    suu, svv, suv = suu - mu * mu, svv - mv * mv, suv - mu * mv
    A2, B2 = 2 * suv + MR.C2, suu + svv + MR.C2
    if cs_only:
        val = A2 / B2
        Du, Dc = -A2 / (B2 * B2), 2 / B2
        Dm = -2 * mu * Du - mv * Dc
    else:
        A1, B1 = 2 * mu * mv + MR.C1, mu * mu + mv * mv + MR.C1
        val = A1 * A2 / (B1 * B2)
        Du, Dc = -A1 * A2 / (B1 * B2 * B2), 2 * A1 / (B1 * B2)
        Dm = 2 * mv * A2 / (B1 * B2) - 2 * mu * A1 * A2 / (B1 * B1 * B2) - 2 * mu * Du - mv * Dc
    wm, wu, wc = torch.zeros_like(u), torch.zeros_like(u), torch.zeros_like(u)
    for dy in range(11):
        for dx in range(11):
            w = g[dy] * g[dx]
            wm[..., dy:dy + IH, dx:dx + IW] += w * Dm
            wu[..., dy:dy + IH, dx:dx + IW] += w * Du
            wc[..., dy:dy + IH, dx:dx + IW] += w * Dc
    return val.sum(dim=(1, 2, 3)), (wm + 2 * u * wu + v * wc) / 2


def closed_form(a, b, weights):
    """The contract without autograd -> (loss, d loss / d a, m [B, M])."""
    M, B, C = len(weights), a.shape[0], a.shape[1]
    pa, pb = [a.double()], [b.double()]
    for _ in range(M - 1):
        pa.append(_pool(pa[-1]))
        pb.append(_pool(pb[-1]))
    sums, dsum, n = [], [], []
    for j in range(M):
        s, ds = _level_closed_form(pa[j], pb[j], j < M - 1)
        sums.append(s), dsum.append(ds), n.append(C * (pa[j].shape[2] - 10) * (pa[j].shape[3] - 10))
    m = torch.stack([s / nj for s, nj in zip(sums, n)], dim=1)
    ok = (m > 0).all(dim=1)
    Pb = torch.zeros(B, dtype=torch.float64)
    for i in range(B):
        if ok[i]:
            Pb[i] = math.prod(float(m[i, j]) ** weights[j] for j in range(M))
    grad = None
    for j in reversed(range(M)):
        k = torch.tensor([weights[j] * float(Pb[i]) / (float(m[i, j]) * B * n[j]) if ok[i] else 0.0 for i in range(B)],
                         dtype=torch.float64)
        gj = -k[:, None, None, None] * dsum[j]
        grad = gj if grad is None else gj + _pool_t(grad, *gj.shape[-2:])
    return 1.0 - Pb.mean(), grad, m


CF_CASES = [((1, 1, 22, 22), None), ((2, 3, 23, 37), None), ((2, 3, 64, 64), None), ((1, 3, 70, 45), None),
            ((1, 1, 11, 300), None), ((2, 3, 64, 64), (0.7, 0.9)), ((1, 1, 45, 47), (0.2, 0.3, 0.5))]


@pytest.mark.parametrize("kind", P.SSIM_KINDS)
@pytest.mark.parametrize("shape,weights", CF_CASES)
def test_restatement_gradient_equals_the_closed_form_with_the_explicit_pooling_adjoint(kind, shape, weights):
    a, b = P.ssim_inputs(kind, *shape)
    w = MR.default_weights(*shape[2:]) if weights is None else weights
    loss, g, m = MR.loss_and_grad(a, b, w)
    lc, gc, mc = closed_form(a, b, w)
    scale, err = float(g.abs().max()), float((gc - g).abs().max())
    print(f"{kind} {shape} M={len(w)}: max |g| {scale:.3e}, closed form - autograd {err:.3e}, loss {float(loss):.6f}")
    assert abs(float(lc) - float(loss)) <= 1e-13 and float((mc - m).abs().max()) <= 1e-13
    clamped = [i for i in range(shape[0]) if not bool((m[i] > 0).all())]
    for i in clamped:                                   # value 0 and gradient exactly 0, in both formulations
        assert not g[i].any() and not gc[i].any()
    if kind == "same":
        assert float(loss) <= 1e-14 and scale <= 1e-13 and float(gc.abs().max()) <= 1e-13     # (see test_ssimloss_cpu.py)
    elif len(clamped) < shape[0]:
        assert scale > 0 and err <= 1e-11 * scale
    else:
        assert float(loss) == 1.0


@pytest.mark.parametrize("H,W", [(23, 37), (11, 11), (12, 13), (45, 70), (33, 64)])
def test_pooling_adjoint_identity_at_odd_sizes(H, W):
    g = P.gen(H * 100 + W)
    x = torch.randn(2, 3, H, W, generator=g, dtype=torch.float64)
    y = torch.randn(2, 3, H // 2, W // 2, generator=g, dtype=torch.float64)
    assert torch.equal(_pool(x), F.avg_pool2d(x, 2)) or float((_pool(x) - F.avg_pool2d(x, 2)).abs().max()) <= 1e-15
    lhs, rhs = float((F.avg_pool2d(x, 2) * y).sum()), float((x * _pool_t(y, H, W)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))
    t = _pool_t(y, H, W)
    assert not t[..., 2 * (H // 2):, :].any() and not t[..., :, 2 * (W // 2):].any()      # dropped rows / columns get nothing
    # autograd agrees: the adjoint IS avg_pool2d's backward
    xr = x.clone().requires_grad_(True)
    (gx,) = torch.autograd.grad((F.avg_pool2d(xr, 2) * y).sum(), xr)
    assert float((gx - t).abs().max()) <= 1e-15


# ======================================================================================================================
# The default-scale rule and the Python layers' argument checks
# ======================================================================================================================
def test_default_scale_rule_from_11_to_10000():
    V = import_module("vaegan_amd")
    f = V.msssim_weights
    assert f is import_module(PKG + ".ops").msssim_weights
    for side in list(range(11, 400)) + [511, 512, 1000, 4096, 10000]:
        want = MR.default_weights(side, side)
        M = len(want)
        assert M == max(m for m in range(1, 6) if (side >> (m - 1)) >= 11)
        for H, W in ((side, side), (side, 3 * side + 1), (10000, side)):
            got = f(H, W)
            assert len(got) == M and all(abs(x - y) <= 1e-15 for x, y in zip(got, want)), (H, W)
            assert abs(sum(got) - 1.0) <= 1e-15
            assert f(H, W, M) == got and len(f(H, W, 1)) == 1 and f(H, W, 1)[0] == 1.0
            if M < 5:
                with pytest.raises(ValueError):
                    f(H, W, M + 1)
                with pytest.raises(ValueError):
                    f(H, W, (0.1,) * (M + 1))
    assert len(f(64, 64)) == 3 and len(f(128, 128)) == 4 and len(f(256, 256)) == 5
    assert [len(f(s, s)) for s in (11, 21, 22, 43, 44, 87, 88, 175, 176)] == [1, 1, 2, 2, 3, 3, 4, 4, 5]
    assert f(256, 256) == tuple(w / sum(MR.PAPER_WEIGHTS) for w in MR.PAPER_WEIGHTS)
    assert f(64, 64, (0.5, 2.0)) == (0.5, 2.0) and f(64, 64, [3.0]) == (3.0,)          # as given, not renormalised
    for bad in (0, 6, -1, (), (0.1,) * 6, (0.5, 0.0), (0.5, -1.0), (float("nan"),), (float("inf"), 1.0), "3", 2.5):
        with pytest.raises(ValueError):
            f(256, 256, bad)
    for H, W in ((10, 64), (64, 10), (0, 0)):
        with pytest.raises(ValueError):
            f(H, W)


def _nets(S=64):
    V = import_module("vaegan_amd")
    return V, V.Encoder([3, S, S], 100), V.Generator(nz=100, img_size=S), V.Discriminator(img_size=S)


def test_keyword_validation_never_reaches_the_device():
    V, e, g, d = _nets()
    with pytest.raises(ValueError, match="alpha_ssim"):
        V.VAEGANTrainer(e, g, d, None, None, None, ssim_scales=3)                      # scales without the term
    with pytest.raises(ValueError, match="alpha_ssim"):
        V.VAETrainer(e, g, None, ssim_scales=3)
    for bad in (0, 6, (), (0.5, -1.0), (float("nan"),), "three", False, 2.5):
        with pytest.raises(ValueError):
            V.VAEGANTrainer(e, g, d, None, None, None, alpha_ssim=1.0, ssim_scales=bad)
        with pytest.raises(ValueError):
            V.VAETrainer(e, g, None, alpha_ssim=1.0, ssim_scales=bad)
    for ok in (True, "auto", 1, 3, (0.3, 0.7)):
        assert V.VAEGANTrainer(e, g, d, None, None, None, alpha_ssim=1.0, ssim_scales=ok).ssim_scales == ok
        assert V.VAETrainer(e, g, None, alpha_ssim=0.5, ssim_scales=ok).ssim_scales == ok
    assert V.VAEGANTrainer(e, g, d, None, None, None).ssim_scales is None
    assert V.VAETrainer(e, g, None).ssim_scales is None
    # the module: bad scales at construction; CPU tensors, other dtypes, small images, a target with a gradient at the call
    for bad in (0, 6, (0.5, 0.0), "x"):
        with pytest.raises(ValueError):
            V.MSSSIMLoss(bad)
    crit = V.MSSSIMLoss()
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(RuntimeError, match="MI355X"):
        crit(x, x)
    ops = import_module(PKG + ".ops")
    with pytest.raises(RuntimeError):
        ops.msssim_loss_forward_backward(x, x, (1.0,), 1.0, torch.zeros(1), False)
    with pytest.raises(RuntimeError):
        ops.ms_ssim(x, x)


# ======================================================================================================================
# ref_step / ref_vae_step
# ======================================================================================================================
def _same_state(a, b):
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_ref_step_without_scales_is_the_single_scale_ref_step_bit_for_bit_and_with_them_swaps_the_term():
    S, B = 64, 2
    a, b, c = (R.RefVAEGAN(img_size=S, seed=42) for _ in range(3))
    inp = make_inputs(B, S, 7000 + S)
    la = SR.ref_step(a, *inp, 60, alpha_ssim=0.5)
    lb = MR.ref_step(b, *inp, 60, ssim_scales=None, alpha_ssim=0.5)
    assert la == lb
    for sa, sb in ((a.E, b.E), (a.G, b.G), (a.D, b.D)):
        _same_state(sa, sb)
    for oa, ob in ((a.opt_E, b.opt_E), (a.opt_G, b.opt_G), (a.opt_D, b.opt_D)):
        assert oa.t == ob.t
        for x, y in zip(oa.exp_avg + oa.exp_avg_sq, ob.exp_avg + ob.exp_avg_sq):
            assert torch.equal(x, y)
    w = MR.default_weights(S, S)
    lc = MR.ref_step(c, *inp, 60, ssim_scales=w, alpha_ssim=0.5)
    for k in ("recon_loss", "kl_loss", "d_loss_1", "d_loss_2", "g_loss_adv"):
        assert la[k] == lc[k]
    assert 0 < lc["ssim_loss"] <= 1 and lc["ssim_loss"] != la["ssim_loss"]
    assert abs(lc["total"] - la["total"] - 0.5 * (lc["ssim_loss"] - la["ssim_loss"])) <= 1e-5 * abs(lc["total"])
    _same_state(a.D, c.D)
    assert not torch.equal(a.opt_G.exp_avg[0], c.opt_G.exp_avg[0])
    # the patch is gone after the step
    assert SR.ssim_loss.__module__ == "_ssimloss_ref"


def test_ref_vae_step_without_scales_is_the_single_scale_step_and_with_them_swaps_the_term():
    S, B = 64, 2
    g = P.gen(8100)
    img = torch.rand(B, 3, S, S, generator=g) * 2 - 1
    eps_img, eps_z = torch.randn(B, 3, S, S, generator=g), torch.randn(B, 100, generator=g)
    a, b, c = (SIB.RefVAE(img_size=S, seed=42) for _ in range(3))
    la = SR.ref_vae_step(a, img, eps_img, eps_z, 25, alpha_ssim=1.0)
    lb = MR.ref_vae_step(b, img, eps_img, eps_z, 25, alpha_ssim=1.0)
    assert la == lb
    _same_state(a.E, b.E), _same_state(a.G, b.G)
    lc = MR.ref_vae_step(c, img, eps_img, eps_z, 25, ssim_scales=MR.default_weights(S, S), alpha_ssim=1.0)
    assert lc["recon_loss"] == la["recon_loss"] and lc["kl_loss"] == la["kl_loss"]
    assert 0 < lc["ssim_loss"] <= 1 and lc["ssim_loss"] != la["ssim_loss"]
    assert not torch.equal(a.opt.exp_avg[0], c.opt.exp_avg[0])


# ======================================================================================================================
# The library: symbols, the workspace query, the host-side argument checks
# ======================================================================================================================
def test_new_symbols_are_declared_bound_and_exported():
    L = import_module(PKG + "._lib")
    lib = L.load()
    src = open(os.path.join(ROOT, "include", "vaegan_hip.h")).read()
    for name in ("vg_msssim_loss_forward_backward", "vg_msssim_ws_bytes"):
        assert name in L.SIGNATURES and name in src
        assert getattr(lib, name) is not None
    assert lib.vg_abi_version() == L.ABI_VERSION
    V = import_module("vaegan_amd")
    for name in ("MSSSIMLoss", "msssim_weights"):
        assert name in V.__all__ and hasattr(V, name) and name in V.__doc__
    assert isinstance(V.MSSSIMLoss(), torch.nn.Module) and isinstance(V.MSSSIMLoss(3), torch.nn.Module)
    ops = import_module(PKG + ".ops")
    assert callable(ops.msssim_loss_forward_backward) and callable(ops.ms_ssim)
    # the timing family the launch-count test reads: valid, and empty while timing is off
    ms, n = ctypes.c_double(-1.0), ctypes.c_int(-1)
    assert lib.vg_timing_collect(5, ctypes.byref(ms), ctypes.byref(n)) == 0 and n.value == 0
    assert lib.vg_timing_collect(6, ctypes.byref(ms), ctypes.byref(n)) == EINVAL


def _expected_bytes(B, C, H, W, M):
    """The layout csrc/msssim.hip documents: f64 [B][1 + M] (P_b and the means), f32 coefficients [B][M], one f32 partial per 32 x 32 tile of every
    level, the pyramids of a and b (levels >= 1) and of the gradient (levels >= 0); every region rounded up to 16 bytes."""
    r4 = lambda v: (v + 3) // 4 * 4
    tiles = sum(B * C * -(-(H >> j) // 32) * -(-(W >> j) // 32) for j in range(M))
    px = [r4(B * C * (H >> j) * (W >> j)) for j in range(M)]
    return 4 * (r4(2 * B * (M + 1)) + r4(B * M) + r4(tiles) + 2 * sum(px[1:]) + sum(px))


def test_workspace_query():
    q = import_module(PKG + "._lib").load().vg_msssim_ws_bytes
    for (shape, M) in MR.GPU_SHAPES + [((128, 3, 64, 64), 3), ((32, 3, 256, 256), 5), ((2, 3, 64, 64), 1), ((2, 3, 64, 64), 2)]:
        got = q(*shape, M)
        assert got > 0 and got % 16 == 0 and got == _expected_bytes(*shape, M), (shape, M, got)
    for bad in ((0, 1, 64, 64, 1), (1, 0, 64, 64, 1), (-1, 3, 64, 64, 1), (1, 1, 10, 64, 1), (1, 1, 64, 10, 1), (1, 1, 0, 0, 1),
                (1, 1, 64, 64, 0), (1, 1, 64, 64, -1), (1, 1, 64, 64, 6), (1, 1, 64, 64, 4), (1, 1, 21, 64, 2),
                (1, 1, 64, 21, 2), (1, 1, 175, 176, 5), (1, 1, 4096, 4096, 6)):
        assert q(*bad) == EINVAL, bad
    assert q(2 ** 15, 2 ** 15, 64, 64, 1) == EINVAL          # more tiles than a launch has workgroups


def test_c_abi_rejects_bad_msssim_arguments_on_host():
    """Validation happens before any launch (pattern: tests/test_ssimloss_cpu.py)."""
    lib = import_module(PKG + "._lib").load()
    f = lib.vg_msssim_loss_forward_backward
    buf = ctypes.c_void_p(4096)
    n = lib.vg_msssim_ws_bytes(2, 3, 64, 64, 3)
    w3 = (ctypes.c_float * 3)(0.1, 0.4, 0.5)
    w5 = (ctypes.c_float * 5)(0.1, 0.2, 0.2, 0.2, 0.3)

    def call(a=buf, b=buf, d=buf, B=2, C=3, H=64, W=64, M=3, w=w3, loss=buf, per=buf, ws=buf, cap=n):
        return f(a, b, d, B, C, H, W, M, w, 1.0, loss, 0, per, ws, cap, None)

    assert f(None, None, None, 0, 0, 0, 0, 0, None, 1.0, None, 0, None, None, 0, None) == EINVAL
    assert call(a=None) == EINVAL and call(b=None) == EINVAL and call(loss=None) == EINVAL
    assert call(d=None, loss=None) == EINVAL                                           # forward only needs the slot too
    assert call(w=None) == EINVAL                                                      # no weights
    for kw in (dict(B=0), dict(B=-2), dict(C=0), dict(C=-3), dict(H=10), dict(W=10),
               dict(M=0), dict(M=-1), dict(M=6, w=w5), dict(M=4, w=w5),               # 64 >> 3 = 8 < 11
               dict(H=43, M=3), dict(W=43, M=3), dict(H=21, M=2), dict(W=21, M=2)):     # a level under 11
        assert call(**kw) == EINVAL, kw
    for bad in (0.0, -0.5, float("nan"), float("inf"), -float("inf")):
        for pos in range(3):
            w = (ctypes.c_float * 3)(0.1, 0.4, 0.5)
            w[pos] = bad
            assert call(w=w) == EINVAL, (bad, pos)
    assert call(ws=None) == EINVAL and call(cap=n - 1) == EINVAL and call(cap=0) == EINVAL and call(cap=-1) == EINVAL
    assert call(B=2 ** 15, C=2 ** 15, M=1, cap=2 ** 62) == EINVAL
    assert call(ws=ctypes.c_void_p(4100)) == -2                                        # VG_EALIGN: the f64 P_b


# ======================================================================================================================
# The input table of the GPU tests
# ======================================================================================================================
@pytest.mark.parametrize("kind", P.SSIM_KINDS)
@pytest.mark.parametrize("shape,M", MR.GPU_SHAPES)
def test_input_table_keeps_every_mean_away_from_the_clamp(kind, shape, M):
    """Kernel and reference must take the same clamp branch: every |m_{b,j}| of the f64 restatement is >= 1e-4, two orders
    above the ~1e-6 an f32 mean can move, and the set of clamped images is the recorded one -- in f64 and in the f32
    evaluation of the same graph (the gradient yardstick).  Smallest: 5.5e-4, noise at (2,1,256,256), image 1 level 4 -- the
    mixed case (one image on the clamp, one not); (2,3,64,64) noise is mixed too."""
    assert MR.default_scales(*shape[2:]) == M
    a, b = P.ssim_inputs(kind, *shape)
    assert a.dtype == torch.float32 and float(a.abs().max()) <= 1 and float(b.abs().max()) <= 1
    m = MR.per_image_means(a, b, M)
    m32 = MR.per_image_means(a, b, M, torch.float32)
    print(f"{kind} {shape}: min |m| {float(m.abs().min()):.3e}")
    assert float(m.abs().min()) >= MR.MIN_ABS_MEAN
    want = MR.clamped(shape, kind)
    assert tuple(i for i in range(shape[0]) if not bool((m[i] > 0).all())) == want
    assert tuple(i for i in range(shape[0]) if not bool((m32[i] > 0).all())) == want
    assert bool(((m > 0) == (m32 > 0)).all())
    if kind == "same":
        assert float((m - 1).abs().max()) <= 1e-12


def test_the_table_holds_the_mixed_and_the_wholly_clamped_cases():
    assert MR.clamped((2, 1, 256, 256), "noise") == (1,) and MR.clamped((2, 3, 64, 64), "noise") == (0,)
    for shape in ((2, 3, 23, 37), (1, 3, 70, 45), (1, 1, 11, 300), (1, 1, 176, 176)):
        assert MR.clamped(shape, "noise") == tuple(range(shape[0]))
    for shape, _ in MR.GPU_SHAPES:
        assert MR.clamped(shape, "negated") == tuple(range(shape[0]))
        for kind in ("same", "small_noise", "constant", "blocks"):
            assert MR.clamped(shape, kind) == ()
    a, b = P.ssim_inputs("noise", 2, 3, 23, 37)
    loss, g, _ = MR.loss_and_grad(a, b, MR.default_weights(23, 37))
    assert float(loss) == 1.0 and not g.any()
