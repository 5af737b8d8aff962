"""GPU: the multi-scale SSIM loss from the kernels up to the trainers and the evaluation passes:
vg_msssim_loss_forward_backward against the f64 restatement of its contract (tests/_msssim_ref.py: torch autograd through
avg_pool2d and the explicit 11 x 11 window form, with the clamp rule), MSSSIMLoss, the iterations of VAEGANTrainer /
VAETrainer with ssim_scales against ref_step / ref_vae_step, and the denoising passes with ms_ssim=True against the loop
written from public pieces.  Bounds: the gradient's is tests/test_gpu_ssimloss.check_grad (4 x the deviation of the same
graph evaluated in f32 by CPU autograd, + U |g|); the loss's is the first-order propagation of the per-level map deviation
through the product.  The input table and its conditions: tests/_msssim_ref.py, asserted in tests/test_msssim_cpu.py.
Parity with the torchmetrics / pytorch-msssim packages is unpinned (neither is installed): the formulas are restated."""
import ctypes
import importlib
import os

import pytest
import torch

import _msssim_ref as MR
import _pointwise_ref as P
import _ssimloss_ref as SR
import siblings_ref as SIB
import vaegan_ref as R
from _inputs import make_inputs
from _pointwise_ref import U

import vaegan_amd as V
from test_gpu_parity import DEV, FIRST_STEP_TOL, oracle_twin_fp64, rel, sync_from_oracle
from test_gpu_siblings import sib_inputs
from test_gpu_ssimloss import (NAN, assert_same_state, build, build_vae, check_grad, full_state, gan_state, guarded,
                               guards_untouched)

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, os.cpu_count() or 1))

PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
ops = importlib.import_module(PKG + ".ops")
L = importlib.import_module(PKG + "._lib")

_REF = {}


def reference(kind, shape, weights=None):
    """Once per case: a, b, the weights, loss64, g64, |g32 - g64| (the gradient yardstick), m64 [B, M], the map deviation per
    level [M] and per (image, level) [B, M]."""
    key = (kind,) + tuple(shape) + (weights,)
    if key not in _REF:
        a, b = P.ssim_inputs(kind, *shape)
        w = MR.default_weights(*shape[2:]) if weights is None else weights
        loss, g, m = MR.loss_and_grad(a, b, w)
        _, g32, _ = MR.loss_and_grad(a, b, w, torch.float32)
        dev_lvl, dev_bm = MR.map_deviation(a, b, len(w))
        _REF[key] = (a, b, w, loss, g, (g32 - g).abs(), m, dev_lvl, dev_bm)
    return _REF[key]


def loss_bound(kind, w, lref, m, dev_lvl):
    """min(4 max_b sum_j (w_j P_b / m_{b,j}) mean|map32_j - map64_j| + U |ref|, 1e-4); `same`: 9 U (8 U per level as for
    vg_ssim, the weights summing to 1, plus the final rounding)."""
    if kind == "same":
        return 9 * U
    Pb = MR.products(m, w)
    sens = max(sum(w[j] * float(Pb[i]) / float(m[i, j]) * float(dev_lvl[j]) for j in range(len(w))) if float(Pb[i]) > 0 else 0.0
               for i in range(m.shape[0]))
    return min(4 * sens + U * abs(float(lref)), 1e-4)


def run(A, Bt, w, gscale, loss, accumulate, d=None, per_scale=None):
    return ops.msssim_loss_forward_backward(A, Bt, w, gscale, loss, accumulate, d, per_scale)


# ======================================================================================================================
# The kernels against the f64 restatement of the contract
# ======================================================================================================================
@pytest.mark.parametrize("kind", P.SSIM_KINDS)
@pytest.mark.parametrize("shape,M", MR.GPU_SHAPES)
def test_msssim_kernel_vs_f64_restatement(kind, shape, M):
    """Achieved error / bound on an MI355X, worst over the seven shapes (gradient, mean or max, zeroed and accumulating d;
    every ratio is printed): noise 0.03, same 0.27 (the true gradient is 0: the kernel leaves max
    1.3e-10 at (2,3,64,64) against 4 dev32_max = 4.9e-10), negated 0 (every image on the clamp: loss 1 and gradient 0,
    exactly), small_noise 0.02, constant 0.03, blocks 0.28; loss <= 0.01 of its bound, per_scale <= 0.02 of 4 dev + U |m|.
    The coarse levels do not eat the margin of 4: the f32 CPU graph loses most through the global coefficient k ~ 1 / m,
    whose means carry the unshifted cancellation; the kernel's shifted maps and f64 sums do not."""
    a, b, w, lref, gref, dev32, m64, dev_lvl, dev_bm = reference(kind, shape)
    assert len(w) == M
    Bn = shape[0]
    A, Bt = a.to(DEV), b.to(DEV)
    what = f"msssim {kind} {'x'.join(map(str, shape))} M={M}"
    clamped = MR.clamped(shape, kind)

    # ---- forward + backward into a zeroed d, gscale 1; d sits between NaN guards (ragged tiles write nothing outside)
    buf, d, guard = guarded(shape, 0.0)
    loss = torch.full((1,), 3.0, device=DEV)
    per = torch.full((Bn, M), NAN, device=DEV)
    assert run(A, Bt, w, 1.0, loss, False, d, per) is d
    got_loss = float(loss)
    lb = loss_bound(kind, w, lref, m64, dev_lvl)
    print(f"{what}: loss {got_loss:.8f} ref {float(lref):.8f} err/bound {abs(got_loss - float(lref)) / lb:.3f}")
    assert abs(got_loss - float(lref)) <= lb
    check_grad(d, gref, gref, dev32, 1.0, what + " grad")
    assert guards_untouched(buf, guard)
    if kind != "same" and len(clamped) < Bn:
        assert float(d.abs().max()) > 0

    # ---- per_scale: the restatement's means within the map deviation, the same sign everywhere
    pm = per.double().cpu()
    pb = 4 * dev_bm + U * m64.abs()
    print(f"{what}: per_scale err/bound {float(((pm - m64).abs() / pb.clamp_min(1e-300)).max()):.3f}")
    assert bool(torch.isfinite(pm).all()) and bool(((pm - m64).abs() <= pb).all())
    assert bool(((pm > 0) == (m64 > 0)).all())
    if kind == "same":
        assert bool((pm == 1.0).all()) and got_loss == 0.0            # numerator and denominator are the same operations

    # ---- accumulation: d pre-filled with storage-exact values comes back as d + gscale grad; clamped images bit for bit
    gs = 0.37
    d0 = (torch.randn(shape, generator=P.gen(sum(shape))) * 1e-3).float()
    buf2, d2, _ = guarded(shape, d0.to(DEV))
    loss2 = torch.full((1,), 3.0, device=DEV)
    run(A, Bt, w, gs, loss2, True, d2)
    dref = SR.grad_add(gref, d0, gs)
    check_grad(d2, dref, P.f32(gs) * gref, dev32, P.f32(gs), what + f" d + {gs} grad", summed=True)
    assert guards_untouched(buf2, guard)
    for i in clamped:                                                # value 0 and gradient exactly 0: d is not touched
        assert torch.equal(d2[i].cpu(), d0[i]) and not d[i].any()
    assert float(loss2) == float(torch.tensor(3.0) + loss.cpu()[0])  # accumulate_loss; gscale does not touch the loss
    if len(clamped) == Bn:
        assert got_loss == 1.0

    # ---- d = NULL: the same loss bits and no write anywhere
    slots = torch.full((8,), NAN, device=DEV)
    idle, _, _ = guarded(shape)
    assert run(A, Bt, w, 1.0, slots[3:4], False, None) is None
    assert float(slots[3]) == got_loss and int(torch.isnan(slots).sum()) == 7
    assert bool(torch.isnan(idle).all()) and guards_untouched(buf, guard)
    run(A, Bt, w, 1.0, slots[3:4], True, None)
    assert float(slots[3]) == float(loss.cpu()[0] + loss.cpu()[0]) and int(torch.isnan(slots).sum()) == 7

    # ---- run to run: the same bits
    loss3, d3, per3 = torch.zeros(1, device=DEV), torch.zeros(shape, device=DEV), torch.zeros(Bn, M, device=DEV)
    run(A, Bt, w, 1.0, loss3, False, d3, per3)
    assert torch.equal(loss3, loss) and torch.equal(d3, d) and torch.equal(per3, per)
    # ---- ms_ssim: 1 - the loss
    assert float(ops.ms_ssim(A, Bt)) == float(torch.tensor(1.0) - loss.cpu()[0])


@pytest.mark.parametrize("kind", ["noise", "small_noise", "blocks"])
def test_explicit_unnormalised_weights_two_scales_at_64(kind):
    shape, w = (2, 3, 64, 64), (0.7, 0.9)
    a, b, w, lref, gref, dev32, m64, dev_lvl, dev_bm = reference(kind, shape, w)
    A, Bt = a.to(DEV), b.to(DEV)
    loss, d, per = torch.zeros(1, device=DEV), torch.zeros(shape, device=DEV), torch.zeros(2, 2, device=DEV)
    run(A, Bt, w, 1.0, loss, False, d, per)
    lb = loss_bound(kind, w, lref, m64, dev_lvl)
    print(f"{kind}: loss {float(loss):.8f} ref {float(lref):.8f} err/bound {abs(float(loss) - float(lref)) / lb:.3f}")
    assert abs(float(loss) - float(lref)) <= lb
    check_grad(d, gref, gref, dev32, 1.0, f"msssim {kind} weights {w} grad")
    assert bool(((per.double().cpu() - m64).abs() <= 4 * dev_bm + U * m64.abs()).all())
    assert float(ops.ms_ssim(A, Bt, w)) == float(torch.tensor(1.0) - loss.cpu()[0])


@pytest.mark.parametrize("shape,M", [((2, 3, 23, 37), 2), ((2, 3, 64, 64), 3), ((2, 1, 256, 256), 5)])
def test_eager_equals_graph_replay_bit_for_bit(shape, M):
    a, b, w, *_ = reference("small_noise" if M < 5 else "noise", shape)
    A, Bt = a.to(DEV), b.to(DEV)
    d0 = (torch.randn(shape, generator=P.gen(5)) * 1e-3).to(DEV)
    loss_e, d_e, per_e = torch.zeros(1, device=DEV), d0.clone(), torch.zeros(shape[0], M, device=DEV)
    run(A, Bt, w, 0.5, loss_e, False, d_e, per_e)                     # (also sizes the workspace before the capture)
    loss_g, d_g, per_g = torch.zeros(1, device=DEV), d0.clone(), torch.zeros(shape[0], M, device=DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(A, Bt, w, 0.5, loss_g, False, d_g, per_g)
    for _ in range(2):
        d_g.copy_(d0)
        loss_g.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss_g, loss_e) and torch.equal(d_g, d_e) and torch.equal(per_g, per_e)


@pytest.mark.parametrize("shape,M,with_d,without_d", [((1, 1, 11, 300), 1, 4, 2), ((2, 3, 64, 64), 3, 5, 3),
                                                      ((1, 1, 176, 176), 5, 5, 3)])
def test_launch_count_does_not_grow_with_the_number_of_scales(shape, M, with_d, without_d):
    """pyramid (M > 1) + forward + finalize (+ backward + collapse): read through vg_timing_collect (family 5 brackets every
    launch of csrc/msssim.hip) and through the library's launch counter."""
    a, b, w, *_ = reference("small_noise", shape)
    assert len(w) == M
    A, Bt = a.to(DEV), b.to(DEV)
    loss, d = torch.zeros(1, device=DEV), torch.zeros(shape, device=DEV)
    run(A, Bt, w, 1.0, loss, False, d)                                # workspace sized, kernels loaded
    torch.cuda.synchronize()
    want = torch.cat([loss, d.flatten()]).cpu()
    lib = L.load()
    ms, n = ctypes.c_double(0.0), ctypes.c_int(0)
    lib.vg_timing_enable(1)
    try:
        for dd, expect in ((d, with_d), (None, without_d)):
            d.zero_()
            n0 = ops.launch_count()
            run(A, Bt, w, 1.0, loss, False, dd)
            assert ops.launch_count() - n0 == expect
            assert lib.vg_timing_collect(5, ctypes.byref(ms), ctypes.byref(n)) == 0
            print(f"{shape} M={M} d={'yes' if dd is not None else 'no'}: {n.value} launches, {ms.value * 1e3:.1f} us")
            assert n.value == expect and ms.value > 0
    finally:
        lib.vg_timing_enable(0)
    d.zero_()
    run(A, Bt, w, 1.0, loss, False, d)
    assert torch.equal(torch.cat([loss, d.flatten()]).cpu(), want)    # timed launches compute the same bits


def test_msssim_wrappers_reject_what_the_kernels_do_not_take():
    a = torch.zeros(1, 1, 32, 32, device=DEV)
    loss = torch.zeros(1, device=DEV)
    w1, w2 = (1.0,), (0.5, 0.5)
    for bad_a, bad_b, bad_w, bad_d, bad_per in (
            (a.cpu(), a.cpu(), w1, None, None), (a, a.double(), w1, None, None), (a.half(), a.half(), w1, None, None),
            (a, a[..., :31].contiguous(), w1, None, None), (a, a, w1, torch.zeros(1, 1, 32, 31, device=DEV), None),
            (a[..., :10].contiguous(), a[..., :10].contiguous(), w1, None, None),              # W < 11
            (a[:, :, :10].contiguous(), a[:, :, :10].contiguous(), w1, None, None),            # H < 11
            (a[..., :21].contiguous(), a[..., :21].contiguous(), w2, None, None),              # the second level under 11
            (a, a, (0.5,) * 3, None, None),                                                    # 32 >> 2 = 8
            (a, a, (), None, None), (a, a, (0.1,) * 6, None, None), (a, a, (0.5, -0.5), None, None),
            (a, a, (float("nan"),), None, None), (a, a, w2, None, torch.zeros(1, 1, device=DEV)),
            (a, a, w2, None, torch.zeros(1, 2, device=DEV, dtype=torch.float64)), (a[0], a[0], w1, None, None)):
        with pytest.raises(RuntimeError):
            ops.msssim_loss_forward_backward(bad_a, bad_b, bad_w, 1.0, loss, False, bad_d, bad_per)
    with pytest.raises(ValueError):
        ops.ms_ssim(a[..., :10].contiguous(), a[..., :10].contiguous())
    assert float(ops.ms_ssim(a, a)) == 1.0


# ======================================================================================================================
# MSSSIMLoss
# ======================================================================================================================
@pytest.mark.parametrize("kind", ["small_noise", "noise"])
def test_msssim_loss_module_value_and_gradient(kind):
    shape = (2, 3, 64, 64)
    a, b, w, lref, gref, dev32, m64, dev_lvl, _ = reference(kind, shape)
    crit = V.MSSSIMLoss()
    x = a.to(DEV).requires_grad_(True)
    t = b.to(DEV)
    loss = crit(x, t)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.requires_grad
    assert abs(float(loss) - float(lref)) <= loss_bound(kind, w, lref, m64, dev_lvl)
    loss.backward()
    check_grad(x.grad, gref, gref, dev32, 1.0, f"MSSSIMLoss {kind} input.grad")
    x2 = a.to(DEV).requires_grad_(True)
    (crit(x2, t) * 2.5).backward()
    assert torch.equal(x2.grad, x.grad * 2.5)
    check_grad(x2.grad, 2.5 * gref, 2.5 * gref, dev32, 2.5, f"MSSSIMLoss {kind} 2.5 x", summed=True)
    # the scales argument: an int and explicit weights reach the kernel as msssim_weights gives them
    assert float(V.MSSSIMLoss(3)(x.detach(), t)) == float(loss)
    assert float(V.MSSSIMLoss(V.msssim_weights(64, 64))(x.detach(), t)) == float(loss)
    if kind == "small_noise":
        # one scale of weight 1 and no image on the clamp: the SSIM loss itself (the same maps, another summation order)
        l1 = torch.zeros(1, device=DEV)
        ops.ssim_loss_forward_backward(x.detach(), t, 1.0, l1, False)
        m1 = float(V.MSSSIMLoss(1)(x.detach(), t))
        print(f"M = 1: {m1:.8f}, the SSIM loss {float(l1):.8f}")
        assert abs(m1 - float(l1)) <= 4 * U


def test_msssim_loss_module_rejects_cpu_non_f32_small_images_and_a_target_with_a_gradient():
    crit = V.MSSSIMLoss()
    a = torch.zeros(1, 3, 32, 32, device=DEV)
    with pytest.raises(RuntimeError, match="MI355X"):
        crit(a.cpu(), a.cpu())
    with pytest.raises(RuntimeError, match="MI355X"):
        crit(a, a.cpu())
    with pytest.raises(TypeError, match="float32"):
        crit(a.bfloat16(), a.bfloat16())
    with pytest.raises(TypeError, match="float32"):
        crit(a, a.double())
    with pytest.raises(ValueError, match="11 x 11"):
        crit(a[..., :10], a[..., :10])
    with pytest.raises(ValueError, match="11 x 11"):
        crit(a[:, :, :10], a[:, :, :10])
    with pytest.raises(ValueError, match="scales"):
        V.MSSSIMLoss(3)(a, a)                                         # 32 >> 2 = 8
    with pytest.raises(ValueError, match="shape"):
        crit(a, a[:, :2])
    with pytest.raises(NotImplementedError):
        crit(a, a.clone().requires_grad_(True))
    assert float(crit(a, a)) == 0.0


# ======================================================================================================================
# The trainers: off means off
# ======================================================================================================================
@pytest.mark.parametrize("graphed", [False, True])
@pytest.mark.parametrize("alpha", [0.0, 1.0])
def test_no_scales_is_bitwise_the_trainer_without_the_argument(graphed, alpha):
    res = []
    for kw in (dict(alpha_ssim=alpha), dict(alpha_ssim=alpha, ssim_scales=None)):
        e, g, d, tr = build(64, **kw)
        fn = tr.train_step_graphed if graphed else tr.train_step
        n0 = ops.launch_count()
        losses = []
        for step in range(3):
            real, ez, er, ec = (t.to(DEV) for t in make_inputs(4, 64, 7064 + step))
            losses.append(fn(real, 60, ez, er, ec).cpu().clone())
        res.append((losses, gan_state(e, g, d, tr), ops.launch_count() - n0, tr.loss_dict(epoch=60)))
    for x, y in zip(res[0][0], res[1][0]):
        assert x.numel() == 8 and torch.equal(x, y)
    assert_same_state(res[0][1], res[1][1])
    assert res[0][2] == res[1][2] and res[0][3] == res[1][3]


@pytest.mark.parametrize("graphed", [False, True])
@pytest.mark.parametrize("alpha", [0.0, 1.0])
def test_no_scales_is_bitwise_the_vae_trainer_without_the_argument(graphed, alpha):
    res = []
    for kw in (dict(alpha_ssim=alpha), dict(alpha_ssim=alpha, ssim_scales=None)):
        e, g, tr = build_vae(64, **kw)
        fn = tr.step_graphed if graphed else tr.train_step
        n0 = ops.launch_count()
        losses = []
        for step in range(3):
            img, eps_img, eps_z, _ = sib_inputs(4, 64, step)
            losses.append(fn(img.to(DEV), eps_img.to(DEV), eps_z.to(DEV), epoch=60).cpu().clone())
        res.append((losses, full_state((e, g), (tr.opt,)), ops.launch_count() - n0))
    for x, y in zip(res[0][0], res[1][0]):
        assert x.numel() == 4 and torch.equal(x, y)
    assert_same_state(res[0][1], res[1][1])
    assert res[0][2] == res[1][2]


# ======================================================================================================================
# The iterations against ref_step / ref_vae_step
# ======================================================================================================================
def test_first_step_with_the_multi_scale_term_vs_ref_step():
    """S = 64, B = 4, fp32, epoch 60, alpha_ssim = 1, the default three scales.  Every loss within FIRST_STEP_TOL; ssim_loss
    takes recon_loss's 1e-4 (the same tensors, before any update).  Image 3 of this input sits on the clamp (m_{3,0} =
    -3.0e-3): the mixed case inside a training step."""
    o = R.RefVAEGAN(img_size=64, seed=42)
    inp = make_inputs(4, 64, 7064)
    w = MR.default_weights(64, 64)
    ref = MR.ref_step(o, *inp, 60, ssim_scales=w, alpha_ssim=1.0)
    e, g, d, tr = build(64, alpha_ssim=1.0, ssim_scales=True)
    real, ez, er, ec = (t.to(DEV) for t in inp)
    out = tr.train_step(real, 60, ez, er, ec)
    got = tr.loss_dict(out, 60)
    tol = dict(FIRST_STEP_TOL, ssim_loss=FIRST_STEP_TOL["recon_loss"])
    print({k: f"{got[k]:.6g} / {ref[k]:.6g} ({rel(got[k], ref[k]):.1e})" for k in tol})
    assert sorted(got) == sorted(tol)
    for k, t in tol.items():
        assert rel(got[k], ref[k]) <= t, f"{k}: hip {got[k]} ref_step {ref[k]}"
    assert float(out[6]) == got["ssim_loss"] > 0 and float(out[5]) == 0.0 and float(out[7]) == 0.0
    # an int and the explicit weights select the same launches; single-scale differs
    for scales in (3, w):
        e, g, d, tr2 = build(64, alpha_ssim=1.0, ssim_scales=scales)
        assert torch.equal(tr2.train_step(real, 60, ez, er, ec), out)
    e, g, d, tr1 = build(64, alpha_ssim=1.0)
    assert float(tr1.train_step(real, 60, ez, er, ec)[6]) != float(out[6])
    want = got["recon_loss"] + 0.1 * got["kl_loss"] + 0.1 * got["g_loss_adv"] + got["ssim_loss"]
    assert abs(got["total"] - want) <= 1e-12 * abs(want)


def test_vae_first_step_with_the_multi_scale_term_vs_ref_vae_step():
    """The denoising VAE, S = 64, B = 4, fp32, epoch 25: losses within 1e-4 (pure forward passes of the initial weights).
    Image 1 of this input sits on the clamp (m_{1,0} = -1.1e-2); the smallest |m| is 1.2e-3."""
    B, S, alpha = 4, 64, 0.5
    img, eps_img, eps_z, _ = sib_inputs(B, S, 0)
    w = MR.default_weights(S, S)
    ref = MR.ref_vae_step(SIB.RefVAE(img_size=S, seed=42), img, eps_img, eps_z, 25, ssim_scales=w, alpha_ssim=alpha)
    e, g, tr = build_vae(S, alpha_ssim=alpha, ssim_scales="auto")
    got = tr.train_step(img.to(DEV), eps_img.to(DEV), eps_z.to(DEV), epoch=25).tolist()
    assert len(got) == 4
    for i, n in enumerate(("recon_loss", "kl_loss", "total", "ssim_loss")):
        print(f"{n}: hip {got[i]:.6g} ref {ref[n]:.6g} ({rel(got[i], ref[n]):.1e})")
        assert rel(got[i], ref[n]) <= 1e-4, f"VAE {n}: hip {got[i]} ref {ref[n]}"
    assert got[3] > 0 and abs(got[2] - (got[0] + 0.5 * 1e-5 * got[1] + alpha * got[3])) <= 4 * U * got[2]


def test_multi_scale_gradient_path_in_isolation_vs_fp64_ref_step():
    """tests/test_gpu_ssimloss.test_ssim_gradient_path_in_isolation_vs_fp64_ref_step with the term swapped: epoch 0, alpha_adv
    = alpha_pix = 0, alpha_ssim = 1, lr = 0 -- every gradient that reaches the Generator and the Encoder comes out of the
    multi-scale kernels.  Same input (its choice depends on the forward alone), same bound per tensor: max error relative
    to the tensor's max <= max(1e-5, 4 x the CPU-fp32 ref_step's own error against the fp64 one).  No image of this input
    is on the clamp (smallest m: 1.9e-3)."""
    S, B = 64, 4
    kw = dict(alpha_adv=0.0, alpha_pix=0.0, alpha_ssim=1.0)
    w = MR.default_weights(S, S)
    e, g, d, tr = build(S, lr=0.0, ssim_scales=True, **kw)
    o = R.RefVAEGAN(img_size=S, seed=42, lr=0.0)
    sync_from_oracle(o, e, g, d, tr)
    o64 = oracle_twin_fp64(o)
    inp = make_inputs(B, S, SR.ISO_SEED)
    MR.ref_step(o64, *inp, 0, ssim_scales=w, **kw)
    MR.ref_step(o, *inp, 0, ssim_scales=w, **kw)
    real, ez, er, ec = (t.to(DEV) for t in inp)
    tr.train_step(real, 0, ez, er, ec)
    worst = 0.0
    for m, opt, st, st64 in ((e, tr.opt_E, o.E, o64.E), (g, tr.opt_G, o.G, o64.G)):
        hsd = opt.state_dict()["state"]
        keys = R.trainable_keys(st)
        assert len(keys) == len(hsd)
        for i, k in enumerate(keys):
            if k.endswith("conv.bias") and m is e:
                continue                    # exactly-zero true gradient in front of BatchNorm: rounding noise everywhere
            r64, r32 = st64[k].grad.double(), st[k].grad.double()
            hip = hsd[i]["exp_avg"].double().cpu().reshape(r64.shape) / (1 - opt.betas[0])
            scale = float(r64.abs().max())
            assert scale > 0, k
            err_hip, err_cpu = float((hip - r64).abs().max()) / scale, float((r32 - r64).abs().max()) / scale
            worst = max(worst, err_hip / max(1e-5, 4 * err_cpu))
            assert err_hip <= max(1e-5, 4 * err_cpu), f"{k}: hip err {err_hip:.2e}, cpu-fp32 err {err_cpu:.2e}"
    print(f"worst gradient error / bound {worst:.3f}")


# ======================================================================================================================
# Graph replay, the capture key, the paired step
# ======================================================================================================================
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_graphed_equals_eager_with_scales_and_recaptures_when_they_change(dtype):
    B, S = 4, 64
    (ee, ge, de, te), (eg, gg, dg, tg) = (build(S, dtype=dtype, alpha_ssim=1.0, ssim_scales=True) for _ in range(2))
    inputs = [[t.to(DEV) for t in make_inputs(B, S, 7064 + step)] for step in range(3)]

    def three_steps():
        out = []
        for real, ez, er, ec in inputs:
            le = te.train_step(real, 60, ez, er, ec).cpu().clone()
            lg = tg.train_step_graphed(real, 60, ez, er, ec).cpu().clone()
            assert torch.equal(le, lg), (le, lg)
            out.append(le)
        assert_same_state(gan_state(ee, ge, de, te), gan_state(eg, gg, dg, tg))
        return out

    first = three_steps()
    assert all(0 < float(l[6]) <= 1 for l in first)
    graph1 = tg._graph
    assert graph1 is not None and len(graph1[1]) == 1            # eager, capture + replay, replay: ONE graph
    te.ssim_scales = tg.ssim_scales = 2                          # the weights are frozen in the graph: re-capture
    second = three_steps()
    assert tg._graph is not graph1 and tg._graph.key != graph1.key
    graph2 = tg._graph
    te.ssim_scales = tg.ssim_scales = None                       # back to the single-scale launches
    third = three_steps()
    assert tg._graph is not graph2 and tg._graph.key != graph2.key and tg._graph.key != graph1.key
    print([float(x[0][6]) for x in (first, second, third)])
    assert len({float(x[0][6]) for x in (first, second, third)}) == 3


def test_vae_graphed_equals_eager_with_scales_and_recaptures_when_they_change():
    B, S = 4, 64
    res = []
    for graphed in (False, True):
        e, g, tr = build_vae(S, alpha_ssim=1.0, ssim_scales=True)
        fn = tr.step_graphed if graphed else tr.train_step
        outs, states = [], []
        for scales in (True, (0.4, 0.6)):
            tr.ssim_scales = scales
            for step in range(3):
                img, eps_img, eps_z, _ = sib_inputs(B, S, step)
                outs.append(fn(img.to(DEV), eps_img.to(DEV), eps_z.to(DEV), epoch=60).clone())
            if graphed:
                assert tr._gstate is not None
                states.append(tr._gstate)
        res.append((torch.stack(outs).cpu(), full_state((e, g), (tr.opt,))))
        if graphed:
            assert states[0] is not states[1] and states[0].key != states[1].key
    assert torch.equal(res[0][0], res[1][0]) and bool((res[0][0][:, 3] > 0).all())
    assert_same_state(res[0][1], res[1][1])


@pytest.mark.parametrize("graphed", [False, True])
def test_paired_step_targets_the_clean_image(graphed):
    """noisy= feeds the Encoder; the multi-scale term, like the single-scale one, compares the reconstruction with `clean`:
    slot 6 equals 1 - ms_ssim(recon, clean) of the reconstruction that step produced (denoise path, train-mode BatchNorm)."""
    B, S = 4, 64
    real, ez, er, ec = (t.to(DEV) for t in make_inputs(B, S, 7064))
    noisy = (real + 0.3 * torch.randn(real.shape, generator=P.gen(3)).to(DEV)).clamp(-1, 1)
    e, g, d, tr = build(S, alpha_ssim=1.0, ssim_scales=True)
    recon = V.denoise_eval(e, g, real, noisy=noisy, eps_z=ez)["recon"]          # the networks are in train mode: the step's forward
    want = float(torch.tensor(1.0) - ops.ms_ssim(recon, real).cpu()[0])
    fn = tr.train_step_graphed if graphed else tr.train_step
    outs = [fn(real, 60, ez, er, ec, noisy=noisy).cpu().clone() for _ in range(3 if graphed else 1)]
    print(float(outs[0][6]), want)
    assert abs(float(outs[0][6]) - want) <= 1e-5 and 0 < float(outs[0][6]) <= 1
    e2, g2, d2, tr2 = build(S, alpha_ssim=1.0, ssim_scales=True)
    unpaired = tr2.train_step(real, 60, ez, er, ec).cpu()
    assert float(unpaired[6]) != float(outs[0][6])
    # the VAE trainer
    img, eps_img, eps_z, _ = (t.to(DEV) if torch.is_tensor(t) else t for t in sib_inputs(B, S, 0))
    nz = (img + 0.3 * torch.randn(img.shape, generator=P.gen(4)).to(DEV)).clamp(-1, 1)
    ev, gv, tv = build_vae(S, alpha_ssim=1.0, ssim_scales=True)
    recon = V.denoise_eval(ev, gv, img, noisy=nz, eps_z=eps_z)["recon"]
    want = float(torch.tensor(1.0) - ops.ms_ssim(recon, img).cpu()[0])
    fv = tv.step_graphed if graphed else tv.train_step
    got = [fv(img, None, eps_z, noisy=nz, epoch=60).cpu().clone() for _ in range(3 if graphed else 1)]
    assert abs(float(got[0][3]) - want) <= 1e-5 and 0 < float(got[0][3]) <= 1


# ======================================================================================================================
# The evaluation passes
# ======================================================================================================================
def eval_nets(S=64):
    V.configure_seed(42)
    e = V.Encoder([3, S, S], 100)
    g = V.Generator(nz=100, img_size=S)
    g.apply(V.weights_init)
    e.to(DEV), g.to(DEV)
    return e, g


def batches(sizes, S, seed):
    gen = P.gen(seed)
    return [(torch.rand(b, 3, S, S, generator=gen) * 2 - 1).to(DEV) for b in sizes]


def same_but(a, b, extra):
    """Dicts a (default) and b (ms_ssim=True): b = a + the extra keys, every common value identical."""
    assert sorted(b) == sorted(list(a) + list(extra)), (sorted(a), sorted(b))
    for k, v in a.items():
        assert (torch.equal(v, b[k]) if torch.is_tensor(v) else v == b[k]), k


def test_validation_epoch_and_denoise_eval_report_ms_ssim():
    S, sizes = 64, (3, 2)
    e, g = eval_nets(S)
    imgs = batches(sizes, S, 50)
    draws = [(torch.randn(x.shape, generator=P.gen(60 + i)).to(DEV), torch.randn(x.shape[0], 100, generator=P.gen(70 + i)).to(DEV))
             for i, x in enumerate(imgs)]
    noise_fn = lambda i, img: draws[i]
    base = V.validation_epoch(e, g, imgs, noise_fn=noise_fn)
    assert sorted(base) == sorted(["val_loss", "ssim", "psnr", "recon_loss", "kl_loss", "samples", "batches"])
    assert V.validation_epoch(e, g, imgs, noise_fn=noise_fn, ms_ssim=False) == base
    out = V.validation_epoch(e, g, imgs, noise_fn=noise_fn, ms_ssim=True)
    same_but(base, out, ["ms_ssim"])
    tot = 0.0
    for x, (eps, eps_z) in zip(imgs, draws):                     # the loop from public pieces (eval mode, as the pass left it)
        one_base = V.denoise_eval(e, g, x, eps=eps, eps_z=eps_z)
        one = V.denoise_eval(e, g, x, eps=eps, eps_z=eps_z, ms_ssim=True)
        same_but(one_base, one, ["ms_ssim"])
        assert sorted(one_base) == sorted(["noisy", "recon", "recon_loss", "kl_loss", "val_loss", "psnr", "ssim"])
        assert one["ms_ssim"] == float(ops.ms_ssim(one["recon"], x))
        assert one["ms_ssim"] == float(1.0 - V.MSSSIMLoss()(one["recon"], x))
        tot += x.shape[0] * one["ms_ssim"]
    print(out["ms_ssim"], tot / sum(sizes), out["ssim"])
    assert abs(out["ms_ssim"] - tot / sum(sizes)) <= 1e-6 * max(abs(out["ms_ssim"]), 1e-3)      # f32 accumulation on the device
    assert 0 <= out["ms_ssim"] <= 1


def test_paired_and_tiled_passes_report_ms_ssim_and_ms_ssim_noisy():
    S, sizes = 64, (3, 2)
    e, g = eval_nets(S)
    clean = batches(sizes, S, 51)
    noisy = [(c + 0.1 * torch.randn(c.shape, generator=P.gen(80 + i)).to(DEV)).clamp(-1, 1) for i, c in enumerate(clean)]
    zs = [torch.randn(c.shape[0], 100, generator=P.gen(90 + i)).to(DEV) for i, c in enumerate(clean)]
    pairs = list(zip(noisy, clean))
    noise_fn = lambda i, n: zs[i]
    base = V.paired_test_epoch(e, g, pairs, noise_fn=noise_fn)
    assert sorted(base) == sorted(["test_loss", "recon_loss", "kl_loss", "ssim", "psnr", "ssim_noisy", "psnr_noisy", "samples",
                                   "batches"])
    assert V.paired_test_epoch(e, g, pairs, noise_fn=noise_fn, ms_ssim=False) == base
    out = V.paired_test_epoch(e, g, pairs, noise_fn=noise_fn, ms_ssim=True)
    same_but(base, out, ["ms_ssim", "ms_ssim_noisy"])
    tr_, tn_ = 0.0, 0.0
    for (n_, c_), z in zip(pairs, zs):
        recon = V.denoise_eval(e, g, c_, noisy=n_, eps_z=z)["recon"]
        tr_ += c_.shape[0] * float(ops.ms_ssim(recon, c_))
        tn_ += c_.shape[0] * float(ops.ms_ssim(n_, c_))
    print(out["ms_ssim"], tr_ / 5, out["ms_ssim_noisy"], tn_ / 5)
    assert abs(out["ms_ssim"] - tr_ / 5) <= 1e-6 * max(abs(tr_ / 5), 1e-3)
    assert abs(out["ms_ssim_noisy"] - tn_ / 5) <= 1e-6 * abs(tn_ / 5) and out["ms_ssim_noisy"] > out["ms_ssim"]

    # ---- the tiled passes: 80 x 101 images through the 64 x 64 networks; the default scales of THAT size (3: 80 >> 2 = 20)
    big = batches((1, 2), 80, 52)
    big = [torch.nn.functional.pad(x, (0, 21), value=0.25) for x in big]             # [b, 3, 80, 101]
    bign = [(c + 0.1 * torch.randn(c.shape, generator=P.gen(95 + i)).to(DEV)).clamp(-1, 1) for i, c in enumerate(big)]
    kw = dict(stride=48, sample=False)
    tb = V.tiled_test_epoch(e, g, zip(bign, big), **kw)
    assert sorted(tb) == sorted(["psnr", "ssim", "recon_loss", "psnr_noisy", "ssim_noisy", "samples", "tiles"])
    to = V.tiled_test_epoch(e, g, zip(bign, big), ms_ssim=True, **kw)
    same_but(tb, to, ["ms_ssim", "ms_ssim_noisy"])
    tr_, tn_ = 0.0, 0.0
    for n_, c_ in zip(bign, big):
        r_ = V.denoise_tiled(e, g, n_, **kw)
        tr_ += c_.shape[0] * float(ops.ms_ssim(r_, c_))
        tn_ += c_.shape[0] * float(ops.ms_ssim(n_, c_))
    assert abs(to["ms_ssim"] - tr_ / 3) <= 1e-6 * max(abs(tr_ / 3), 1e-3) and abs(to["ms_ssim_noisy"] - tn_ / 3) <= 1e-6 * abs(tn_ / 3)
    eb = V.tiled_denoise_eval(e, g, big[1], noisy=bign[1], **kw)
    eo = V.tiled_denoise_eval(e, g, big[1], noisy=bign[1], ms_ssim=True, **kw)
    same_but(eb, eo, ["ms_ssim", "ms_ssim_noisy"])
    assert eo["ms_ssim"] == float(ops.ms_ssim(eo["recon"], big[1])) and eo["ms_ssim_noisy"] == float(ops.ms_ssim(bign[1], big[1]))
    assert eo["ms_ssim"] == float(ops.ms_ssim(eo["recon"], big[1], V.msssim_weights(80, 101)))
