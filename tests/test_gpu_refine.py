"""GPU: test-time latent refinement from the kernels up -- vg_bn_act_backward_eval bit for bit on exact inputs and within
its counted roundings on random ones, vg_masked_mse_rows and vg_latent_adam against the restatements of tests/_refine_ref.py,
the eval-mode backward of the engine against f64 autograd, LatentRefiner against the f64 loop (graphed and eager, row
independence, the Discriminator term, bf16) and paired_test_epoch(refine=)."""
import importlib
import math
import os

import numpy as np
import pytest
import torch

import _pairloss_ref as PR
import _refine_ref as RR

import vaegan_amd as V
from test_gpu_data import jpeg_folder  # noqa: F401  (fixture: 45 generated 64 x 64 JPEGs)

pytestmark = pytest.mark.gpu
DEV = "cuda"
torch.set_num_threads(min(16, os.cpu_count() or 1))

PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
G = importlib.import_module(PKG + ".geometry")
ops = importlib.import_module(PKG + ".ops")
data = importlib.import_module(PKG + ".data")
engine = importlib.import_module(PKG + ".engine")
U = 2.0 ** -24                      # unit roundoff of f32
U16 = 2.0 ** -8                     # ... of bf16 (8 significant bits)
F32, BF16 = G.F32, G.BF16
TDT = {F32: torch.float32, BF16: torch.bfloat16}

# Deviation of the refined latent from the f64 loop of tests/_refine_ref.py (S = 16, B = 4, steps = 5, lr = 0.05, fp32 engine),
# max over every element, as measured on an MI355X; the tests assert 8 x it, for the spread between
# machines.  Adam divides by sqrt(v): an f32 rounding of a gradient moves an iterate by about lr x its relative error.
TRAJ_DEV_MEASURED = 3.9041e-3       # context loss only; with the Discriminator term 1.0088e-3; objectives 8.3e-6 / 2.9e-6
TRAJ_BOUND = 8 * TRAJ_DEV_MEASURED


# ======================================================================================================================
# (a) vg_bn_act_backward_eval
# ======================================================================================================================
def _dev(t, dtype, misalign=0):
    """numpy f32 [rows, C] -> a device tensor in the storage type; misalign: its base that many ELEMENTS past a 256-byte
    boundary (4 bf16 = 8 bytes: off the 16-byte grid, on the 8-byte one)."""
    t = torch.from_numpy(np.ascontiguousarray(t)).to(TDT[dtype])
    if not misalign:
        return t.to(DEV)
    buf = torch.empty(t.numel() + misalign, dtype=t.dtype, device=DEV)
    out = buf[misalign:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 != 0
    return out


def _run_eval(x, dy, scale, shift, act, slope, dtype, misalign=0):
    """-> dx as f32 numpy; the destination is NaN-filled and sits between two sentinel rows that must survive."""
    rows, C = x.shape
    X, DY = _dev(x, dtype, misalign), _dev(dy, dtype)
    co = torch.zeros(1, 4, C, device=DEV)
    co[0, 2], co[0, 3] = torch.from_numpy(scale).to(DEV), torch.from_numpy(shift).to(DEV)
    guard = torch.full((rows + 2, C), float("nan"), dtype=TDT[dtype], device=DEV)
    guard[0], guard[-1] = 7.0, -7.0
    out = ops.bn_act_backward_eval(X, DY, co, rows, C, act, slope, dtype, out=guard[1:-1])
    assert out.data_ptr() == guard[1].data_ptr()
    assert bool((guard[0] == 7.0).all()) and bool((guard[-1] == -7.0).all()), "a sentinel row was written"
    return guard[1:-1].float().cpu().numpy()


@pytest.mark.parametrize("dtype,misalign", [(F32, 0), (BF16, 0), (BF16, 4)], ids=["f32", "bf16_16byte", "bf16_4wide_misaligned"])
@pytest.mark.parametrize("rows,C", [(r, c) for r in (1, 37, 300) for c in (8, 24, 264)] + [(37, 12)])
def test_bn_act_backward_eval_is_bitwise_on_exact_inputs(rows, C, dtype, misalign):
    """Power-of-two scales, small integers, halves (tests/_refine_ref.exact_case; z == 0 in row 0): every operation is exact, the
    reference is unique, the comparison bitwise.  C = 12 keeps bf16 on the 4-wide path on aligned pointers as well."""
    x, dy, scale, shift = RR.exact_case(100 + rows + C, rows, C)
    for act in (RR.ACT_NONE, RR.ACT_RELU, RR.ACT_LRELU):
        want = RR.bn_act_backward_eval(x, dy, scale, shift, act, RR.EXACT_SLOPE, bf16=dtype == BF16)
        got = _run_eval(x, dy, scale, shift, act, RR.EXACT_SLOPE, dtype, misalign)
        assert not np.isnan(got).any(), "an element was not written"
        assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want)), (act, np.abs(got - want).max())


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_bn_act_backward_eval_random_inputs_within_the_counted_roundings(dtype):
    """dy * slope and * scale are two f32 roundings ((1 + U)^2), the store one more in bf16; the mask is the restatement's (the
    same fused z).  Against the exact f64 value of the expression."""
    rng = np.random.default_rng(9)
    rows, C = 300, 264
    x, dy = (RR.bf16_round(rng.standard_normal((rows, C)).astype(np.float32)) for _ in range(2))
    scale, shift = (rng.standard_normal(C) + 0.2).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    slope = 0.2
    for act in (RR.ACT_NONE, RR.ACT_RELU, RR.ACT_LRELU):
        got = _run_eval(x, dy, scale, shift, act, slope, dtype)
        z = (x.astype(np.float64) * scale + shift).astype(np.float32)
        dz = dy.astype(np.float64) if act == RR.ACT_NONE else np.where(z > 0, dy, dy * (float(np.float32(slope)) if act == RR.ACT_LRELU else 0.0))
        exact = dz * scale
        bound = (2.5 * U + (U16 if dtype == BF16 else 0.0)) * np.abs(exact)
        err = np.abs(got - exact)
        print(f"act {act} dtype {dtype}: worst err/bound {float((err[bound > 0] / bound[bound > 0]).max()):.3f}")
        assert (err <= bound).all()
        assert np.array_equal(got, RR.bn_act_backward_eval(x, dy, scale, shift, act, slope, bf16=dtype == BF16))


def test_bn_act_backward_eval_wrapper_rejects_mismatched_tensors():
    x = torch.zeros(4, 8, device=DEV)
    co = torch.zeros(1, 4, 8, device=DEV)
    for bad in (dict(coeffs=torch.zeros(2, 4, 8, device=DEV)), dict(coeffs=torch.zeros(1, 4, 16, device=DEV)), dict(coeffs=None),
                dict(dy=x.bfloat16()), dict(dy=torch.zeros(4, 4, device=DEV)), dict(out=torch.zeros(4, 4, device=DEV))):
        kw = dict(x=x, dy=x, coeffs=co, rows=4, C=8, act=1, slope=0.0, dtype=F32)
        kw.update(bad)
        with pytest.raises(RuntimeError, match="bn_act_backward_eval"):
            ops.bn_act_backward_eval(**kw)


# ======================================================================================================================
# (b) vg_masked_mse_rows
# ======================================================================================================================
def _mm_inputs(shape):
    g = torch.Generator().manual_seed(200 + sum(shape))
    a, b = torch.rand(shape, generator=g) * 2 - 1, torch.rand(shape, generator=g) * 2 - 1
    a.view(-1)[::7] = b.view(-1)[::7]              # planted: a == b, the gradient there is exactly 0
    return a, b


def _misaligned(t):
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4
    return out


@pytest.mark.parametrize("shape,misalign", [((3, 3, 16, 16), False), ((3, 3, 16, 18), False), ((3, 3, 16, 16), True),
                                            ((5, 3, 64, 64), False)],
                         ids=["16x16_vec", "16x18_scalar", "16x16_misaligned_base", "64x64_several_workgroups"])
def test_masked_mse_rows_vs_f64_restatement(shape, misalign):
    """Bounds counted as for vg_region_mse_forward_backward (tests/test_gpu_pairloss.py): q = fl(fl(a - b)^2) carries
    (1 + U)^3 - 1, the f64 sum and the rounding of the quotient less than 2 U more: loss_rows within 5 U; a gradient element
    within 4 U |g_ref| (the rounding of d, of the coefficient, of their product).  The rectangle table is that file's
    (cycle_rects: empty, full image, 1 x 1 corners, edges inside a vector, clipped, a NaN row) over three shifts, and NULL."""
    Bn, C, H, W = shape
    a, b = _mm_inputs(shape)
    A, Bt = (_misaligned(a.to(DEV)), b.to(DEV)) if misalign else (a.to(DEV), b.to(DEV))
    for shift in (0, 3, 6, None):
        rects_h = None if shift is None else PR.offset_rects(Bn, H, W, shift)
        rects = None if rects_h is None else rects_h.to(DEV)
        for gs in (1.0, 0.37):
            ref_l, ref_g, n_valid = RR.masked_mse_rows(a, b, rects_h, gs)
            rows = torch.full((Bn,), 3.0, device=DEV)
            d = ops.masked_mse_rows(A, Bt, rects, gs, rows, True)
            got_l, got_g = rows.double().cpu(), d.double().cpu()
            worst = float(((got_l - ref_l).abs() / (5 * U * ref_l).clamp(min=1e-300)).max())
            print(f"{shape} shift={shift} gscale={gs}: loss err/bound {worst:.3f}")
            assert bool(torch.isfinite(got_l).all()) and bool(((got_l - ref_l).abs() <= 5 * U * ref_l).all())
            assert bool(((got_g - ref_g).abs() <= 4 * U * ref_g.abs()).all())
            hole = PR.region_mask(rects_h, *shape)
            assert float(got_g[hole].abs().max() if hole.any() else 0.0) == 0.0 and float(got_g.view(-1)[::7].abs().max()) == 0.0
            assert all(float(got_l[i]) == 0.0 for i in range(Bn) if int(n_valid[i]) == 0)
            # the zero pattern is that of the region kernel with w_hole = 0 on the same inputs
            dr = ops.region_mse_forward_backward(A, Bt, rects, 0.0, gs, want_grad=True)
            assert torch.equal(d == 0, dr == 0)
            # two runs: the same bits; each output alone: the same bits
            rows2 = torch.full((Bn,), 3.0, device=DEV)
            d2 = ops.masked_mse_rows(A, Bt, rects, gs, rows2, True)
            assert torch.equal(rows2, rows) and torch.equal(d2, d)
            rows3 = torch.full((Bn,), 3.0, device=DEV)
            assert ops.masked_mse_rows(A, Bt, rects, gs, rows3, False) is None and torch.equal(rows3, rows)
            assert torch.equal(ops.masked_mse_rows(A, Bt, rects, gs, None, True), d)


def test_masked_mse_rows_an_image_never_sees_another_images_partials():
    a, b = _mm_inputs((5, 3, 64, 64))
    rects_h = PR.offset_rects(5, 64, 64, 2)
    A, Bt, rects = a.to(DEV), b.to(DEV), rects_h.to(DEV)
    rows = torch.empty(5, device=DEV)
    d = ops.masked_mse_rows(A, Bt, rects, 1.0, rows, True)
    perm = [4, 1, 3, 2, 0]
    rows_p = torch.empty(5, device=DEV)
    d_p = ops.masked_mse_rows(A[perm].contiguous(), Bt[perm].contiguous(), rects[perm].contiguous(), 1.0, rows_p, True)
    assert torch.equal(rows_p, rows[perm]) and torch.equal(d_p, d[perm])
    with pytest.raises(RuntimeError, match="masked_mse_rows"):
        ops.masked_mse_rows(A, Bt, rects[:4].contiguous(), 1.0, rows, True)
    with pytest.raises(RuntimeError, match="masked_mse_rows"):
        ops.masked_mse_rows(A, Bt, rects, 1.0, None, False)


# ======================================================================================================================
# (c) vg_latent_adam
# ======================================================================================================================
def _state_np(st):
    return {k: v.cpu().numpy() for k, v in st.items()}


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B", [1, 5])
def test_latent_adam_three_steps_vs_the_restatement(B, dtype):
    """The kernel forms every stored value in f64 from f32 state and rounds once, and so does the restatement: what can differ
    is the last bit of an f64 library function (log) before that rounding -- one f32 ulp (2 U relative) on z, m, v and J; the
    engine-type copy one bf16 ulp.  INIT, three UPDATEs (with p and the prior term), then TRACK."""
    L, ZP = 100, G.padc(100, dtype)
    bf = dtype == BF16
    rng = np.random.default_rng(40 + B)
    kw = dict(lr=0.05, betas=(0.9, 0.999), eps=1e-8, alpha_adv=0.1, prior_weight=0.3)
    z0 = np.zeros((B, ZP), np.float32)
    z0[:, :L] = rng.standard_normal((B, L))
    z0 = RR.bf16_round(z0) if bf else z0
    ref = RR.LatentAdam(B, L, ZP, bf16=bf)
    want_out = ref.init(z0)
    st = ops.latent_state(B, L, DEV)
    z_eng = torch.full((B, ZP), float("nan"), dtype=TDT[dtype], device=DEV)
    ops.latent_adam("init", st, dtype, ZP, z_in=torch.from_numpy(z0).to(TDT[dtype]).to(DEV), z_out=z_eng)
    s = _state_np(st)
    assert np.array_equal(s["z"], ref.z) and np.array_equal(s["best_z"], ref.z) and not s["m"].any() and not s["v"].any()
    assert not s["t"].any() and np.isinf(s["best_loss"]).all() and np.array_equal(z_eng.float().cpu().numpy(), want_out)

    def close(got, want, what, ulp=2 * U):
        err = np.abs(got.astype(np.float64) - want.astype(np.float64))
        assert np.isfinite(got).all() and (err <= ulp * np.abs(want)).all(), (what, float(err.max()))

    obj = torch.empty(B, device=DEV)
    for k in range(3):
        dz = rng.standard_normal((B, ZP)).astype(np.float32) * 0.05
        dz = RR.bf16_round(dz) if bf else dz
        loss = rng.random(B).astype(np.float32)
        p = rng.random(B).astype(np.float32) * 0.98 + 0.01
        J, want_out = ref.update(dz, loss, p, **kw)
        ops.latent_adam("update", st, dtype, ZP, dz=torch.from_numpy(dz).to(TDT[dtype]).to(DEV), loss_rows=torch.from_numpy(loss).to(DEV),
                        p=torch.from_numpy(p).to(DEV), z_out=z_eng, objective=obj, **kw)
        s = _state_np(st)
        for name in ("z", "m", "v", "best_z"):
            close(s[name], getattr(ref, name), (k, name))
        close(s["best_loss"], ref.best_loss, (k, "best_loss"))
        close(obj.cpu().numpy(), J, (k, "objective"))
        assert s["t"].tolist() == [k + 1] * B
        out = z_eng.float().cpu().numpy()
        assert not out[:, L:].any() and np.array_equal(np.signbit(out[:, L:]), np.zeros((B, ZP - L), bool)), "padding lanes: +0"
        close(out[:, :L], want_out[:, :L], (k, "z_out"), 2 * U16 if bf else 2 * U)
        if not bf:
            assert np.array_equal(out[:, :L], s["z"])
    before = _state_np(st)
    # lower than anything before (the prior term alone was larger): TRACK takes it, and moves nothing else
    loss = np.full(B, 1e-3, np.float32)
    ref.track(loss, None, 0.0, 0.0)
    ops.latent_adam("track", st, dtype, ZP, loss_rows=torch.from_numpy(loss).to(DEV), objective=obj)
    assert obj.tolist() == loss.tolist()
    s = _state_np(st)
    for name in ("z", "m", "v", "t"):
        assert np.array_equal(s[name], before[name]), name
    assert np.array_equal(s["best_z"], s["z"])
    close(s["best_loss"], ref.best_loss, "track best_loss")


def test_latent_adam_row_counters_ties_and_nan():
    B, L, ZP = 3, 100, 100
    st = ops.latent_state(B, L, DEV)
    z0 = torch.randn(B, ZP, generator=torch.Generator().manual_seed(1)).to(DEV)
    z_eng = torch.empty(B, ZP, device=DEV)
    ops.latent_adam("init", st, F32, ZP, z_in=z0, z_out=z_eng)
    dz = torch.ones(B, ZP, device=DEV)
    nan = float("nan")
    ops.latent_adam("update", st, F32, ZP, dz=dz, loss_rows=torch.tensor([1.0, 2.0, nan], device=DEV), z_out=z_eng, lr=0.05)
    assert st["best_loss"].tolist()[:2] == [1.0, 2.0] and math.isinf(st["best_loss"][2].item())
    assert torch.equal(st["best_z"], z0[:, :L]), "the best z is the one that was evaluated"
    z1 = st["z"].clone()
    assert not torch.equal(z1, z0[:, :L])
    # rows advance on their own: a second update that only sees rows 0..1 (a view of the state) leaves row 2 at t = 1
    sub = {k: v[:2] for k, v in st.items()}
    ops.latent_adam("update", sub, F32, ZP, dz=dz[:2], loss_rows=torch.tensor([1.0, 1.5], device=DEV), z_out=z_eng[:2], lr=0.05)
    assert st["t"].tolist() == [2, 2, 1]
    assert st["best_loss"].tolist()[:2] == [1.0, 1.5] and math.isinf(st["best_loss"][2].item())       # a tie keeps the earlier iterate
    assert torch.equal(st["best_z"][0], z0[0, :L]) and torch.equal(st["best_z"][1], z1[1]) and torch.equal(st["best_z"][2], z0[2, :L])
    ops.latent_adam("track", st, F32, ZP, loss_rows=torch.tensor([nan, nan, 0.5], device=DEV))
    assert st["best_loss"].tolist() == [1.0, 1.5, 0.5] and torch.equal(st["best_z"][2], st["z"][2])
    # p = 0: nn.BCELoss' clamp, -max(log 0, -100) = 100
    obj = torch.empty(B, device=DEV)
    ops.latent_adam("track", st, F32, ZP, loss_rows=torch.zeros(B, device=DEV), p=torch.tensor([0.0, 1.0, 0.5], device=DEV),
                    objective=obj, alpha_adv=0.1)
    assert obj[0].item() == pytest.approx(10.0, rel=1e-6) and obj[1].item() == 0.0 and obj[2].item() == pytest.approx(0.1 * math.log(2), rel=1e-6)
    with pytest.raises(RuntimeError, match="latent_adam"):
        ops.latent_adam("update", st, F32, ZP, dz=dz, loss_rows=None, z_out=z_eng)
    with pytest.raises(ValueError, match="mode"):
        ops.latent_adam("step", st, F32, ZP)


# ======================================================================================================================
# The engine's eval-mode backward
# ======================================================================================================================
def _nets_on_device(nets, dtype="fp32", with_d=True):
    g = V.Generator(nz=nets.L, img_size=nets.S, dtype=dtype)
    g.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in nets.G.items()})
    d = None
    if with_d:
        d = V.Discriminator(img_size=nets.S, dtype=dtype)
        d.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in nets.D.items()})
        d.to(DEV)
    return g.to(DEV), d


def _snapshot(*mods):
    return [(n, t.detach().clone()) for m in mods for n, t in list(m.named_parameters()) + list(m.named_buffers())]


def _assert_untouched(snap, *mods):
    now = [(n, t) for m in mods for n, t in list(m.named_parameters()) + list(m.named_buffers())]
    assert len(now) == len(snap)
    for (n, a), (n2, b) in zip(snap, now):
        assert n == n2 and torch.equal(a, b.detach()), n
    assert all(p.grad is None for m in mods for p in m.parameters()), "a .grad appeared"


@pytest.fixture(scope="module")
def nets():
    return RR.Nets()


class _F32Nets:
    """The f64 restated networks run in f32 on the CPU: what calibrates an fp32 gradient's own error."""

    def __init__(self, nets):
        self.n = nets
        self.G = {k: v.float() if v.is_floating_point() else v for k, v in nets.G.items()}
        self.D = {k: v.float() if v.is_floating_point() else v for k, v in nets.D.items()}

    def grads(self, z, d_recon, dp, dtype):
        import vaegan_ref as R
        n = self.n
        Gs, Ds = (n.G, n.D) if dtype == torch.float64 else (self.G, self.D)
        zr = z.to(dtype).requires_grad_(True)
        recon = R.generator_forward(Gs, n.g_spec, zr[:, :, None, None], False)
        p = R.discriminator_forward(Ds, n.d_spec, recon, False)
        d_img, = torch.autograd.grad((p * dp.to(dtype)).sum(), recon, retain_graph=True)
        dz, = torch.autograd.grad((recon * d_recon.to(dtype)).sum() + (p * dp.to(dtype)).sum(), zr)
        return dz.double(), d_img.double(), recon.detach().double(), p.detach().double()


def test_engine_eval_mode_backward_vs_f64_autograd(nets):
    """Generator and Discriminator at img_size = 16, B = 2, fp32.  Tolerance: the one of the fp32 gradient parity test,
    tests/test_gpu_parity.test_all_parameter_gradients_vs_fp64_oracle -- per tensor, max error relative to the tensor's max
    <= max(1e-5, 4 x the CPU-fp32 run's own error against fp64)."""
    B, L, S = 2, nets.L, nets.S
    g, d = _nets_on_device(nets)
    gen = torch.Generator().manual_seed(77)
    z, d_recon, dp = torch.randn(B, L, generator=gen), torch.randn(B, 3, S, S, generator=gen) * 0.01, torch.randn(B, generator=gen)
    ref = _F32Nets(nets)
    dz64, dimg64, recon64, p64 = ref.grads(z, d_recon, dp, torch.float64)
    dz32, dimg32, recon32, p32 = ref.grads(z, d_recon, dp, torch.float32)
    snap = _snapshot(g, d)
    ZP, CP = G.padc(L, F32), G.padc(3, F32)
    sink = engine.GradSink(direct=False)
    pre, ctxG = g._engine.forward(ops.prior_forward(z.to(DEV), B, L, ZP, F32), B, False, keep=True)
    recon = ops.nhwc_to_nchw(pre, 3, F32, apply_tanh=True)
    p, ctxD = d._engine.forward(ops.nchw_to_nhwc(recon, CP, F32), B, False, keep=True)
    d_img =d._engine.backward(ctxD, dp.to(DEV), True, sink, param_grads=False)
    d_pre = ops.nchw_grad_add_to_nhwc(d_recon.to(DEV), d_img, recon, CP, F32)
    dz = g._engine.backward(ctxG, d_pre, True, sink, param_grads=False)
    assert not sink.out, "a parameter gradient was formed"
    got_img = d_img.view(B, S, S, CP)[..., :3].permute(0, 3, 1, 2).double().cpu()
    got_dz = dz.view(B, ZP)[:, :L].double().cpu()
    for name, got, r64, r32 in (("image", recon.double().cpu(), recon64, recon32), ("p", p.double().cpu(), p64, p32),
                                ("image gradient", got_img, dimg64, dimg32), ("dz", got_dz, dz64, dz32)):
        scale = float(r64.abs().max())
        err_hip, err_cpu = float((got - r64).abs().max()) / scale, float((r32 - r64).abs().max()) / scale
        print(f"{name}: hip err {err_hip:.2e}, cpu-fp32 err {err_cpu:.2e}")
        assert scale > 0 and err_hip <= max(1e-5, 4 * err_cpu), f"{name}: hip err {err_hip:.2e}, cpu-fp32 err {err_cpu:.2e}"
    _assert_untouched(snap, g, d)
    assert g._engine.pending_bn_ticks == 0 and d._engine.pending_bn_ticks == 0
    # parameter gradients through an eval-mode context are still refused, with the message of before
    with pytest.raises(RuntimeError, match="eval-mode network is not supported"):
        g._engine.backward(ctxG, d_pre, True, sink)
    with pytest.raises(ValueError, match="eval-mode backward"):
        d._engine.backward(ctxD, dp.to(DEV), True, sink, param_grads=False, weight_grad_groups=2)
    _assert_untouched(snap, g, d)


# ======================================================================================================================
# LatentRefiner
# ======================================================================================================================
STEPS, LR = 5, 0.05


@pytest.fixture(scope="module")
def case(nets):
    noisy, rects, z_star, z0 = RR.make_case(nets)
    loops = {adv: RR.refine_loop(nets, noisy, rects, z0, STEPS, lr=LR, alpha_adv=adv, prior_weight=RR.CASE_PRIOR) for adv in (0.0, 0.1)}
    return noisy, rects, z0, loops


def _refiner(nets, adv=0.0, dtype="fp32", **kw):
    g, d = _nets_on_device(nets, dtype, with_d=adv != 0.0)
    return V.LatentRefiner(None, g, d, steps=STEPS, lr=LR, alpha_adv=adv, prior_weight=RR.CASE_PRIOR, **kw), g, d


def _bound():
    return TRAJ_BOUND


@pytest.mark.parametrize("adv", [0.0, 0.1], ids=["context_only", "with_discriminator"])
def test_refiner_follows_the_f64_loop_and_lowers_every_objective(nets, case, adv):
    noisy, rects, z0, loops = case
    ref = loops[adv]
    r, g, d = _refiner(nets, adv)
    mods = [m for m in (g, d) if m is not None]
    snap = _snapshot(*mods)
    out = r.refine(noisy.to(DEV), rects.to(DEV), init=z0.to(DEV))
    assert set(out) == {"recon", "z", "z0", "recon0", "objective0", "objective", "steps"} and out["steps"] == STEPS
    assert torch.equal(out["z0"].cpu(), z0)
    obj0, obj = out["objective0"].double().cpu(), out["objective"].double().cpu()
    dev_z = float((out["z"].double().cpu() - ref["best_z"]).abs().max())
    dev_o = max(float((obj0 - ref["objectives"][0]).abs().max()), float((obj - ref["best"]).abs().max()))
    print(f"alpha_adv {adv}: max |z - z_f64| = {dev_z:.3e}, max |objective - f64| = {dev_o:.3e}; objective0 {obj0.tolist()} -> {obj.tolist()}")
    assert bool((obj <= obj0).all()), "keep-best: exact by construction"
    assert bool((obj < obj0).all()), "these inputs descend (tests/test_refine_cpu.py asserts it of the f64 loop)"
    assert dev_z <= _bound() and dev_o <= _bound()
    # recon is the decode of the returned latent, recon0 that of z0
    # (tolerance: the one tests/test_gpu_parity.py holds denoise_eval's fp32 reconstruction to)
    with torch.no_grad():
        torch.testing.assert_close(out["recon"].double().cpu(), nets.decode(out["z"].double().cpu()), rtol=1e-3, atol=2e-5)
        torch.testing.assert_close(out["recon0"].double().cpu(), nets.decode(z0.double()), rtol=1e-3, atol=2e-5)
    _assert_untouched(snap, *mods)
    assert all(m.training for m in mods), "the modules' flags are left alone"


def test_refiner_graphed_equals_eager_and_captures_once_per_weights(nets, case):
    noisy, rects, z0, _ = case
    N, Rc, Z0 = noisy.to(DEV), rects.to(DEV), z0.to(DEV)
    rg, g, d = _refiner(nets, 0.1)
    re_ = V.LatentRefiner(None, g, d, steps=STEPS, lr=LR, alpha_adv=0.1, prior_weight=RR.CASE_PRIOR, graphed=False)
    a = rg.refine(N, Rc, init=Z0)
    assert rg.captures == 1
    b = re_.refine(N, Rc, init=Z0)
    assert re_.captures == 0
    for k in ("recon", "z", "z0", "recon0", "objective0", "objective"):
        assert torch.equal(a[k], b[k]), k
    a2 = rg.refine(N, Rc, init=Z0)                       # the second call replays the first capture: the same bits
    assert rg.captures == 1 and all(torch.equal(a[k], a2[k]) for k in ("recon", "z", "objective"))
    # rows are independent: image 0 of [a, b, c, d] and of [a, d, c, b]
    perm = [0, 3, 2, 1]
    c = rg.refine(N[perm].contiguous(), Rc[perm].contiguous(), init=Z0[perm].contiguous())
    assert rg.captures == 1
    for k in ("recon", "z", "recon0", "objective0", "objective"):
        assert torch.equal(c[k][0], a[k][0]), k
    assert torch.equal(c["z"][1], a["z"][3])
    # rects=None is a NaN table: no hole -- another result, the same capture
    e = rg.refine(N, None, init=Z0)
    assert rg.captures == 1 and not torch.equal(e["objective0"], a["objective0"])
    # a changed weight: the engines' pack key moves, the refiner captures again and reads the new operands
    with torch.no_grad():
        g.main[0].weight.mul_(1.01)
    a3 = rg.refine(N, Rc, init=Z0)
    b3 = re_.refine(N, Rc, init=Z0)
    assert rg.captures == 2 and not torch.equal(a3["z"], a["z"])
    assert torch.equal(a3["z"], b3["z"]) and torch.equal(a3["recon"], b3["recon"])
    # keep_best=False returns the last iterate and its own objective
    last = V.LatentRefiner(None, g, d, steps=STEPS, lr=LR, alpha_adv=0.1, prior_weight=RR.CASE_PRIOR, keep_best=False).refine(N, Rc, init=Z0)
    assert bool((a3["objective"] <= last["objective"]).all())
    zero = V.LatentRefiner(None, g, d, steps=0, alpha_adv=0.1, prior_weight=RR.CASE_PRIOR).refine(N, Rc, init=Z0)
    assert torch.equal(zero["z"], Z0) and torch.equal(zero["objective"], zero["objective0"]) and torch.equal(zero["objective0"], a3["objective0"])
    with pytest.raises(ValueError, match="without an encoder"):
        rg.refine(N, Rc)
    with pytest.raises(ValueError, match="init"):
        rg.refine(N, Rc, init=Z0[:, :50])
    with pytest.raises(RuntimeError, match="rects"):
        rg.refine(N, Rc[:2], init=Z0)


def test_refiner_bf16_engine_runs_stays_finite_and_never_raises_the_best_objective(nets, case):
    noisy, rects, z0, _ = case
    r, g, d = _refiner(nets, 0.1, dtype="bf16")
    out = r.refine(noisy.to(DEV), rects.to(DEV), init=z0.to(DEV))
    for k in ("recon", "z", "recon0", "objective0", "objective"):
        assert bool(torch.isfinite(out[k]).all()), k
    print("bf16 objective0", out["objective0"].tolist(), "objective", out["objective"].tolist())
    assert bool((out["objective"] <= out["objective0"]).all())
    assert out["recon"].dtype == torch.float32 and out["z"].dtype == torch.float32


# ======================================================================================================================
# paired_test_epoch(refine=)
# ======================================================================================================================
REFINED_KEYS = {"recon_loss_refined", "ssim_refined", "psnr_refined"}
REGION_REFINED = {k + "_refined" for k in ("mse_hole", "mse_valid", "psnr_hole", "psnr_valid", "hole_fraction")}


def test_paired_test_epoch_refine_keys_equal_the_loop_built_from_public_pieces(jpeg_folder):  # noqa: F811
    S = 64
    V.configure_seed(42)
    e, g, d = V.Encoder([3, S, S], 100), V.Generator(nz=100, img_size=S), V.Discriminator(img_size=S)
    g.apply(V.weights_init), d.apply(V.weights_init)
    e.to(DEV), g.to(DEV), d.to(DEV)
    ds = data.ResidentImages.from_folder(jpeg_folder, device=DEV, workers=1)
    loader = data.DeviceLoader(ds, torch.arange(40, 45), 2, shuffle=False, degrade=data.Degrade(0.25))
    eps = [torch.randn(b, 100, generator=torch.Generator().manual_seed(60 + i)) for i, b in enumerate((2, 2, 1))]
    noise_fn = lambda i, noisy: eps[i].to(DEV)                                  # noqa: E731
    torch.manual_seed(5)
    base = V.paired_test_epoch(e, g, loader, noise_fn=noise_fn)
    torch.manual_seed(5)
    none = V.paired_test_epoch(e, g, loader, noise_fn=noise_fn, refine=None)
    assert none == base and list(none) == list(base), "refine=None: today's keys and numbers, bit for bit"
    kw = dict(steps=3, lr=0.05, alpha_adv=0.1, prior_weight=0.01, discriminator=d)
    snap = _snapshot(e, g, d)
    torch.manual_seed(5)
    got = V.paired_test_epoch(e, g, loader, noise_fn=noise_fn, refine=kw)
    assert set(got) == set(base) | REFINED_KEYS and all(got[k] == base[k] for k in base)
    assert loader._rects is False and loader.last_rects is None, "want_rects is withdrawn"
    torch.manual_seed(5)
    both = V.paired_test_epoch(e, g, loader, noise_fn=noise_fn, refine=V.LatentRefiner(e, g, d, **{k: v for k, v in kw.items() if k != "discriminator"}),
                               regions=True)
    assert REFINED_KEYS | REGION_REFINED <= set(both) and all(both[k] == got[k] for k in REFINED_KEYS)
    assert all(torch.equal(a, b) for (_, a), (_, b) in zip(snap, _snapshot(e, g, d))), "parameters and buffers are untouched"
    # the loop from public pieces
    ref = V.LatentRefiner(e, g, d, **{k: v for k, v in kw.items() if k != "discriminator"})
    loader.want_rects(True)
    torch.manual_seed(5)
    acc_ssim = acc_mse = 0.0
    stats = torch.zeros(4, dtype=torch.float64, device=DEV)
    seen = 0
    for noisy, clean in loader:
        b = clean.shape[0]
        recon = ref.refine(noisy.contiguous(), rects=loader.last_rects)["recon"]
        slot = torch.empty(1, device=DEV)
        ops.mse_forward_backward(recon, clean.contiguous(), 1.0, slot, False)
        acc_mse += b * float(slot)
        acc_ssim += b * float(ops.ssim(recon, clean.contiguous()))
        ops.region_mse_forward_backward(recon, clean.contiguous(), loader.last_rects, 1.0, 1.0, stats=stats)
        seen += b
    loader.want_rects(False)
    s_hole, s_valid, n_hole, n_valid = stats.tolist()
    print("refined", {k: both[k] for k in sorted(REFINED_KEYS | REGION_REFINED)}, "one-shot", base["recon_loss"], base["ssim"])
    # the pass accumulates b * value in f32 on the device, this loop in f64 on the host: a few f32 roundings
    assert both["recon_loss_refined"] == pytest.approx(acc_mse / seen, rel=8 * U)
    assert both["ssim_refined"] == pytest.approx(acc_ssim / seen, rel=8 * U)
    assert both["psnr_refined"] == pytest.approx(10 * math.log10(4.0 / (acc_mse / seen)), abs=1e-4)
    assert both["mse_hole_refined"] == s_hole / n_hole and both["mse_valid_refined"] == s_valid / n_valid
    assert both["hole_fraction_refined"] == n_hole / (n_hole + n_valid) == both["hole_fraction"]
    with pytest.raises(RuntimeError, match="want_rects"):
        V.paired_test_epoch(e, g, [(torch.zeros(1, 3, S, S, device=DEV),) * 2], refine=ref)
