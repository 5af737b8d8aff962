"""GPU: the SSIM reconstruction loss from the kernel up to the trainers: vg_ssim_loss_forward_backward against the f64
restatement of its contract (tests/_ssimloss_ref.py: torch autograd through the explicit 11 x 11 window form), SSIMLoss,
and the iterations of VAEGANTrainer / VAETrainer with alpha_ssim against ref_step / ref_vae_step (the oracles' iterations
with the one term added) -- losses, the gradient path in isolation, off-means-off, hipGraph replay, the capture key and
a checkpoint round trip."""
import importlib
import os

import pytest
import torch

import _pointwise_ref as P
import _ssimloss_ref as SR
import siblings_ref as SIB
import vaegan_ref as R
from _inputs import make_inputs
from _pointwise_ref import U

import vaegan_amd as V
from test_gpu_parity import DEV, FIRST_STEP_TOL, oracle_twin_fp64, rel, sync_from_oracle
from test_gpu_siblings import sib_inputs

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, os.cpu_count() or 1))

PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
ops = importlib.import_module(PKG + ".ops")
NAN = float("nan")


def build(S, dtype="fp32", lr=2e-4, **kw):
    """tests/test_gpu_parity.build with trainer arguments."""
    V.configure_seed(42)
    e = V.Encoder([3, S, S], 100, dtype=dtype)
    g = V.Generator(nz=100, img_size=S, dtype=dtype)
    d = V.Discriminator(img_size=S, dtype=dtype)
    g.apply(V.weights_init)
    d.apply(V.weights_init)
    e.to(DEV), g.to(DEV), d.to(DEV)
    tr = V.VAEGANTrainer(e, g, d, *(V.Adam(m.parameters(), lr=lr) for m in (e, g, d)), **kw)
    tr.train()
    return e, g, d, tr


def build_vae(S, dtype="fp32", **kw):
    """tests/test_gpu_siblings.build_vae with trainer arguments."""
    V.configure_seed(42)
    e = V.Encoder([3, S, S], 100, dtype=dtype)
    g = V.Generator(nz=100, img_size=S, dtype=dtype)
    e.to(DEV), g.to(DEV)
    tr = V.VAETrainer(e, g, V.Adam(list(e.parameters()) + list(g.parameters()), lr=1e-3), **kw)
    tr.train()
    return e, g, tr


def full_state(nets, opts):
    """Every parameter, buffer and Adam moment (+ step counters) on the host."""
    torch.cuda.synchronize()
    out = {}
    for i, m in enumerate(nets):
        for k, v in m.state_dict().items():
            out[f"net{i}.{k}"] = v.cpu().clone()
    for i, o in enumerate(opts):
        for a in ("flat_p", "exp_avg", "exp_avg_sq", "state_dev"):
            out[f"opt{i}.{a}"] = getattr(o, a).cpu().clone()
        out[f"opt{i}.steps"] = torch.tensor(o.steps)
    return out


def gan_state(e, g, d, tr):
    return full_state((e, g, d), (tr.opt_E, tr.opt_G, tr.opt_D))


def assert_same_state(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ======================================================================================================================
# The kernel against the f64 restatement of its contract
# ======================================================================================================================
SSIM_LOSS_SHAPES = [(1, 1, 11, 11),          # one interior pixel, a halo larger than the tile
                    (2, 3, 12, 17),          # small ragged plane
                    (2, 3, 64, 64),          # the project's own plane: 2 x 2 tiles
                    (1, 3, 70, 45),          # ragged tiles both ways (3 x 2 tiles of 32 x 32)
                    (1, 1, 11, 300),         # one interior row, ten tiles
                    (2, 1, 256, 256)]        # 64 tiles per plane.  (No grid cap in the kernel: one workgroup per tile.)
_REF = {}


def reference(kind, shape):
    """(a, b, loss64, g64, dev32 of the gradient: |f32 autograd - f64 autograd|, dev32 of the SSIM map: mean), once per case."""
    key = (kind,) + shape
    if key not in _REF:
        a, b = P.ssim_inputs(kind, *shape)
        loss, g = SR.loss_and_grad(a, b)
        _, g32 = SR.loss_and_grad(a, b, torch.float32)
        dev_map = float((P.ssim_map(a, b, torch.float32).double() - P.ssim_map(a, b)).abs().mean())
        _REF[key] = (a, b, loss, g, (g32 - g).abs(), dev_map)
    return _REF[key]


def guarded(shape, fill=None):
    """A tensor of `shape` in the middle of a NaN-filled buffer -> (buffer, view, guard length)."""
    n = int(torch.tensor(shape).prod())
    guard = shape[-1] * shape[-2] + 64
    buf = torch.full((n + 2 * guard,), NAN, device=DEV)
    view = buf[guard:guard + n].view(shape)
    if fill is not None:
        view.copy_(torch.as_tensor(fill, dtype=torch.float32).expand(shape))
    return buf, view, guard


def guards_untouched(buf, guard):
    return bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[-guard:]).all())


def check_grad(got, ref, g, dev32, scale, what, summed=False):
    """The issue's bound, measured the way tests/test_gpu_pointwise.py measures the metric's: the f32 arithmetic is a
    cancellation (E[x^2] - E[x]^2 against c2 = 9e-4) that cannot be bounded from the formula, so the yardstick is the
    deviation `dev32` of the SAME textbook graph evaluated in f32 by torch autograd on the CPU from the f64 one:
        mean |got - ref| <= 4 scale mean(dev32) + U mean|g|,   max |got - ref| <= 4 scale max(dev32) + U max|g|
    with g the (scaled) gradient; ref = g unless the gradient was added onto values already in d or multiplied once more,
    and then (summed) the one further f32 rounding of that result joins the bound: + U mean|ref| / U max|ref|."""
    got = got.detach().double().cpu()
    err, g = (got - ref).abs(), g.abs()
    bm = 4 * scale * float(dev32.mean()) + U * float(g.mean()) + (U * float(ref.abs().mean()) if summed else 0.0)
    bx = 4 * scale * float(dev32.max()) + U * float(g.max()) + (U * float(ref.abs().max()) if summed else 0.0)
    rm, rx = float(err.mean()) / max(bm, 1e-300), float(err.max()) / max(bx, 1e-300)
    print(f"{what}: mean err {float(err.mean()):.3e} (/bound {rm:.3f}), max err {float(err.max()):.3e} (/bound {rx:.3f}), "
          f"mean|g| {float(g.mean()):.3e}, dev32 mean {float(dev32.mean()):.3e}")
    assert bool(torch.isfinite(got).all()), what
    assert float(err.mean()) <= bm, f"{what}: mean err / bound {rm:.3f}"
    assert float(err.max()) <= bx, f"{what}: max err / bound {rx:.3f}"


@pytest.mark.parametrize("kind", P.SSIM_KINDS)
@pytest.mark.parametrize("B,C,H,W", SSIM_LOSS_SHAPES)
def test_ssim_loss_kernel_vs_f64_restatement(kind, B, C, H, W):
    """Achieved error / bound on an MI355X, worst over the shapes (every ratio is printed): noise
    0.60, negated 0.55, blocks 0.16, constant 0.04, small_noise 0.02, same 0.98 (the true gradient is 0 there: the kernel
    leaves max 4.1e-11 at (2,3,64,64) against 4 dev32_max = 4.2e-11, the CPU f32 autograd's own residual); loss <= 0.01."""
    shape = (B, C, H, W)
    a, b, lref, gref, dev32, dev_map = reference(kind, shape)
    A, Bt = a.to(DEV), b.to(DEV)
    what = f"ssim loss {kind} {B}x{C}x{H}x{W}"

    # ---- forward + backward into a zeroed d, gscale 1; d sits between NaN guards (ragged tiles write nothing outside)
    buf, d, guard = guarded(shape, 0.0)
    loss = torch.full((1,), 3.0, device=DEV)
    assert ops.ssim_loss_forward_backward(A, Bt, 1.0, loss, False, d) is d
    got_loss = float(loss)
    if kind == "same":
        lbound = 8 * U                                              # as vg_ssim: ssim(a, a) within 8 U of 1
    else:
        lbound = min(4 * dev_map + U * abs(float(lref)), 1e-4)      # as vg_ssim: 4 dev32 of the map, never over 1e-4
    print(f"{what}: loss {got_loss:.8f} ref {float(lref):.8f} err/bound {abs(got_loss - float(lref)) / lbound:.3f}")
    assert abs(got_loss - float(lref)) <= lbound
    check_grad(d, gref, gref, dev32, 1.0, what + " grad")
    assert guards_untouched(buf, guard)
    if kind != "same":
        assert float(d.abs().max()) > 0

    # ---- accumulation: d pre-filled with storage-exact values comes back as d + gscale grad
    gs = 0.37
    d0 = (torch.randn(shape, generator=P.gen(B + C + H + W)) * 1e-3).float()
    buf2, d2, _ = guarded(shape, d0.to(DEV))
    loss2 = torch.full((1,), 3.0, device=DEV)
    ops.ssim_loss_forward_backward(A, Bt, gs, loss2, True, d2)
    dref = SR.grad_add(gref, d0, gs)
    check_grad(d2, dref, P.f32(gs) * gref, dev32, P.f32(gs), what + f" d + {gs} grad", summed=True)
    assert guards_untouched(buf2, guard)
    # accumulate_loss: the slot's value + the very same loss, in f32; gscale does not touch the loss
    assert float(loss2) == float(torch.tensor(3.0) + loss.cpu()[0])

    # ---- d = NULL: the same loss bits and no write anywhere: the slot sits between NaNs, and so does the buffer a
    # gradient would have gone to
    slots = torch.full((8,), NAN, device=DEV)
    idle, _, _ = guarded(shape)
    assert ops.ssim_loss_forward_backward(A, Bt, 1.0, slots[3:4], False, None) is None
    assert float(slots[3]) == got_loss and int(torch.isnan(slots).sum()) == 7
    assert bool(torch.isnan(idle).all()) and guards_untouched(buf, guard)
    ops.ssim_loss_forward_backward(A, Bt, 1.0, slots[3:4], True, None)
    assert float(slots[3]) == float(loss.cpu()[0] + loss.cpu()[0]) and int(torch.isnan(slots).sum()) == 7

    # ---- run to run: the same bits
    loss3, d3 = torch.zeros(1, device=DEV), torch.zeros(shape, device=DEV)
    ops.ssim_loss_forward_backward(A, Bt, 1.0, loss3, False, d3)
    assert torch.equal(loss3, loss) and torch.equal(d3, d)


def test_ssim_loss_wrapper_rejects_what_the_kernel_does_not_take():
    a = torch.zeros(1, 1, 16, 16, device=DEV)
    loss = torch.zeros(1, device=DEV)
    for bad_a, bad_b, bad_d in ((a.cpu(), a.cpu(), None), (a, a.double(), None), (a.half(), a.half(), None),
                                (a, a[..., :15].contiguous(), None), (a, a, torch.zeros(1, 1, 16, 15, device=DEV)),
                                (a[..., :10].contiguous(), a[..., :10].contiguous(), None),        # W < 11
                                (a[:, :, :10].contiguous(), a[:, :, :10].contiguous(), None),      # H < 11
                                (a[0], a[0], None)):
        with pytest.raises(RuntimeError):
            ops.ssim_loss_forward_backward(bad_a, bad_b, 1.0, loss, False, bad_d)


# ======================================================================================================================
# SSIMLoss
# ======================================================================================================================
@pytest.mark.parametrize("kind", ["small_noise", "noise"])
def test_ssim_loss_module_value_and_gradient(kind):
    shape = (2, 3, 64, 64)
    a, b, lref, gref, dev32, dev_map = reference(kind, shape)
    crit = V.SSIMLoss()
    x = a.to(DEV).requires_grad_(True)
    t = b.to(DEV)
    loss = crit(x, t)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.requires_grad
    assert abs(float(loss) - float(lref)) <= min(4 * dev_map + U * abs(float(lref)), 1e-4)
    loss.backward()
    check_grad(x.grad, gref, gref, dev32, 1.0, f"SSIMLoss {kind} input.grad")
    # a non-unit upstream gradient: backward returns g * saved (one more rounding of the product: U |2.5 g|)
    x2 = a.to(DEV).requires_grad_(True)
    (crit(x2, t) * 2.5).backward()
    assert torch.equal(x2.grad, x.grad * 2.5)
    check_grad(x2.grad, 2.5 * gref, 2.5 * gref, dev32, 2.5, f"SSIMLoss {kind} 2.5 x", summed=True)


def test_ssim_loss_module_rejects_cpu_non_f32_and_small_images():
    crit = V.SSIMLoss()
    a = torch.zeros(1, 3, 16, 16, device=DEV)
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
    with pytest.raises(ValueError, match="shape"):
        crit(a, a[:, :2])
    assert float(crit(a, a)) == 0.0


# ======================================================================================================================
# Off means off
# ======================================================================================================================
@pytest.mark.parametrize("graphed", [False, True])
def test_ssim_term_off_is_bitwise_the_trainer_without_the_argument(graphed):
    res = []
    for kw in ({}, dict(alpha_ssim=0.0)):
        e, g, d, tr = build(64, **kw)
        fn = tr.train_step_graphed if graphed else tr.train_step
        n0 = ops.launch_count()
        losses = []
        for step in range(3):
            real, ez, er, ec = (t.to(DEV) for t in make_inputs(4, 64, 7064 + step))
            losses.append(fn(real, 60, ez, er, ec).cpu().clone())
        res.append((losses, gan_state(e, g, d, tr), ops.launch_count() - n0, tr.loss_dict(epoch=60)))
    for a, b in zip(res[0][0], res[1][0]):
        assert a.numel() == 8 and torch.equal(a, b) and float(a[6]) == 0.0       # all 8 slots; slot 6 reads 0 when off
    assert_same_state(res[0][1], res[1][1])
    assert res[0][2] == res[1][2], "the term, switched off, changed the number of kernel launches"
    assert res[0][3] == res[1][3] and "ssim_loss" not in res[1][3]


@pytest.mark.parametrize("graphed", [False, True])
def test_ssim_term_off_is_bitwise_the_vae_trainer_without_the_argument(graphed):
    res = []
    for kw in ({}, dict(alpha_ssim=0.0)):
        e, g, tr = build_vae(64, **kw)
        fn = tr.step_graphed if graphed else tr.train_step
        n0 = ops.launch_count()
        losses = []
        for step in range(3):
            img, eps_img, eps_z, _ = sib_inputs(8, 64, step)
            losses.append(fn(img.to(DEV), eps_img.to(DEV), eps_z.to(DEV), epoch=60).cpu().clone())
        res.append((losses, full_state((e, g), (tr.opt,)), ops.launch_count() - n0))
    for a, b in zip(res[0][0], res[1][0]):
        assert a.numel() == 4 and torch.equal(a, b) and float(a[3]) == 0.0       # slot 3 reads 0 when off
    assert_same_state(res[0][1], res[1][1])
    assert res[0][2] == res[1][2], "the term, switched off, changed the number of kernel launches"


# ======================================================================================================================
# The iterations against ref_step / ref_vae_step
# ======================================================================================================================
def test_first_step_with_the_ssim_term_on_vs_ref_step():
    """S = 64, B = 4, fp32, epoch 60, alpha_ssim = 1.  Every loss within FIRST_STEP_TOL of tests/test_gpu_parity.py; ssim_loss
    is evaluated on the same tensors as recon_loss, before any update, and takes that entry's 1e-4."""
    o = R.RefVAEGAN(img_size=64, seed=42)
    inp = make_inputs(4, 64, 7064)
    ref = SR.ref_step(o, *inp, 60, alpha_ssim=1.0)
    e, g, d, tr = build(64, alpha_ssim=1.0)
    real, ez, er, ec = (t.to(DEV) for t in inp)
    out = tr.train_step(real, 60, ez, er, ec)
    got = tr.loss_dict(out, 60)
    tol = dict(FIRST_STEP_TOL, ssim_loss=FIRST_STEP_TOL["recon_loss"])
    print({k: f"{got[k]:.6g} / {ref[k]:.6g} ({rel(got[k], ref[k]):.1e})" for k in tol})
    assert sorted(got) == sorted(tol)
    for k, t in tol.items():
        assert rel(got[k], ref[k]) <= t, f"{k}: hip {got[k]} ref_step {ref[k]}"
    assert float(out[6]) == got["ssim_loss"] > 0 and float(out[5]) == 0.0 and float(out[7]) == 0.0
    # together with the Discriminator-feature term and a pixel weight: the total carries all of them
    e, g, d, tr = build(64, alpha_ssim=0.5, feat_layer=2, alpha_feat=0.25, alpha_pix=0.5)
    both = tr.loss_dict(tr.train_step(real, 60, ez, er, ec), 60)
    assert both["ssim_loss"] == got["ssim_loss"] and both["feat_loss"] > 0
    want = 0.5 * both["recon_loss"] + 0.1 * both["kl_loss"] + 0.1 * both["g_loss_adv"] + 0.25 * both["feat_loss"] \
        + 0.5 * both["ssim_loss"]
    assert abs(both["total"] - want) <= 1e-12 * abs(want)


def test_vae_first_step_with_the_ssim_term_on_vs_ref_vae_step():
    """The denoising VAE, S = 64, B = 8, fp32, epoch 25: first-iteration losses within 1e-4 (tests/test_gpu_siblings.py:
    pure forward passes of the initial weights); slot 3 carries the unweighted term and total includes alpha_ssim times it."""
    B, S, alpha = 8, 64, 0.5
    img, eps_img, eps_z, _ = sib_inputs(B, S, 0)
    ref = SR.ref_vae_step(SIB.RefVAE(img_size=S, seed=42), img, eps_img, eps_z, 25, alpha_ssim=alpha)
    e, g, tr = build_vae(S, alpha_ssim=alpha)
    got = tr.train_step(img.to(DEV), eps_img.to(DEV), eps_z.to(DEV), epoch=25).tolist()
    assert len(got) == 4
    for i, n in enumerate(("recon_loss", "kl_loss", "total", "ssim_loss")):
        print(f"{n}: hip {got[i]:.6g} ref {ref[n]:.6g} ({rel(got[i], ref[n]):.1e})")
        assert rel(got[i], ref[n]) <= 1e-4, f"VAE {n}: hip {got[i]} ref {ref[n]}"
    assert got[3] > 0 and abs(got[2] - (got[0] + 0.5 * 1e-5 * got[1] + alpha * got[3])) <= 4 * U * got[2]


def test_ssim_gradient_path_in_isolation_vs_fp64_ref_step():
    """epoch = 0 (KL weight 0), alpha_adv = 0, alpha_pix = 0, alpha_ssim = 1, lr = 0: every gradient that reaches the Generator
    and the Encoder comes out of the SSIM kernel (the MSE launch writes zeros, the adversarial branch adds zeros).
    Teacher-forced from the oracle's state; gradient = exp_avg / (1 - beta1) after the first Adam step (the moments move
    with lr = 0 all the same).  Bound per tensor, as tests/test_gpu_parity.test_all_parameter_gradients_vs_fp64_oracle
    calibrates it: max error relative to the tensor's max <= max(1e-5, 4 x the CPU-fp32 ref_step's own error against the
    fp64 one).  The Encoder's conv.bias tensors are skipped for the reason given there (an exactly-zero true gradient in
    front of BatchNorm), and no others.  Fails without the feature (no such argument).
    The input is make_inputs(4, 64, _ssimloss_ref.ISO_SEED), chosen from the fp64 oracle alone: the first seed from 7064 on
    whose forward keeps every ReLU / LeakyReLU pre-activation 2e-6 away from zero (_ssimloss_ref.activation_margin has the
    reasoning, tests/test_ssimloss_cpu.py the check).  On seed 7064 itself two pre-activations lie within 2.5e-7 of zero
    and fp32 forwards take the other branch there: measured on an MI355X with that seed, cnn.0.conv.weight 4.37e-3 off
    the fp64 gradient against 6.97e-4 for the CPU fp32 oracle of that machine (4.37e-3, on every tensor, for the CPU fp32
    oracle of another) -- a property of the input, with the pixel MSE alone just as with this term."""
    S, B = 64, 4
    kw = dict(alpha_adv=0.0, alpha_pix=0.0, alpha_ssim=1.0)
    e, g, d, tr = build(S, lr=0.0, **kw)
    o = R.RefVAEGAN(img_size=S, seed=42, lr=0.0)
    sync_from_oracle(o, e, g, d, tr)
    o64 = oracle_twin_fp64(o)
    assert tr.opt_G.lr == 0.0 and o64.opt_G.lr == 0.0
    inp = make_inputs(B, S, SR.ISO_SEED)
    SR.ref_step(o64, *inp, 0, **kw)
    SR.ref_step(o, *inp, 0, **kw)
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
# Graph replay, the capture key, a checkpoint in the middle
# ======================================================================================================================
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_graphed_equals_eager_with_the_ssim_term_on_and_recaptures_on_change(dtype):
    B, S = 4, 64
    (ee, ge, de, te), (eg, gg, dg, tg) = (build(S, dtype=dtype, alpha_ssim=1.0) for _ in range(2))
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
    assert all(float(l[6]) > 0 for l in first)
    graph1 = tg._graph
    assert graph1 is not None and len(graph1[1]) == 1            # eager, capture + replay, replay: ONE graph
    # a new weight: the next call may not replay the old graph (the scalar is frozen in it)
    te.alpha_ssim = tg.alpha_ssim = 0.25
    second = three_steps()
    assert tg._graph is not graph1 and tg._graph.key != graph1.key
    assert all(float(l[6]) > 0 for l in second)
    print([float(x[0][6]) for x in (first, second)])


def test_vae_graphed_equals_eager_with_the_ssim_term_on():
    B, S = 8, 64
    res = []
    for graphed in (False, True):
        e, g, tr = build_vae(S, alpha_ssim=1.0)
        fn = tr.step_graphed if graphed else tr.train_step
        outs = []
        for step in range(3):
            img, eps_img, eps_z, _ = sib_inputs(B, S, step)
            outs.append(fn(img.to(DEV), eps_img.to(DEV), eps_z.to(DEV), epoch=60).clone())
        res.append((torch.stack(outs).cpu(), full_state((e, g), (tr.opt,))))
        if graphed:
            assert tr._gstate is not None
    assert torch.equal(res[0][0], res[1][0]) and bool((res[0][0][:, 3] > 0).all())
    assert_same_state(res[0][1], res[1][1])


@pytest.mark.parametrize("graphed", [False, True])
def test_checkpoint_round_trip_mid_run_resumes_bitwise_with_the_ssim_term_on(tmp_path, graphed):
    """tests/test_gpu_parity.test_checkpoint_resume_is_bitwise_identical with alpha_ssim = 1."""
    S, B = 64, 4
    ins = [tuple(t.to(DEV) for t in make_inputs(B, S, 700 + i)) for i in range(4)]

    def run(tr, idx):
        fn = tr.train_step_graphed if graphed else tr.train_step
        return [fn(ins[i][0], 60, *ins[i][1:]).clone() for i in idx]

    e, g, d, tr = build(S, alpha_ssim=1.0)
    run(tr, [0, 1])
    path = str(tmp_path / "ck.pth")
    tr.save_checkpoint(path, epoch=60)
    la = run(tr, [2, 3])
    e2, g2, d2, tr2 = build(S, alpha_ssim=1.0)
    with torch.no_grad():
        for m in (e2, g2, d2):
            for p_ in m.parameters():
                p_.add_(1.0)                       # make sure the load is what restores the state
    assert tr2.load_checkpoint(path) == {"epoch": 60}
    lb = run(tr2, [2, 3])
    for a, b in zip(la, lb):
        assert torch.equal(a, b) and float(a[6]) > 0
    assert_same_state(gan_state(e, g, d, tr), gan_state(e2, g2, d2, tr2))
