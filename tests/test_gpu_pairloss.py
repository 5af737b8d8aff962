"""GPU: training on degraded pairs from the kernel up -- vg_region_mse_forward_backward against the f64 restatement of its
contract (tests/_pairloss_ref.py), its mask against the degradation kernel's rectangle, the loader's want_rects / bind_noisy,
the paired VAE-GAN and VAE iterations against ref_step / ref_vae_step (losses, the gradient path, hipGraph replay, the
capture key), "paired with nothing to pair" against the unpaired step bit for bit, and paired_test_epoch(regions=True)."""
import importlib
import math
import os

import pytest
import torch

import _pairloss_ref as PR
import _ssimloss_ref as SR
import siblings_ref as SIB
import vaegan_ref as R
from _inputs import make_inputs
from _pairloss_ref import U

import vaegan_amd as V
from test_gpu_data import jpeg_folder  # noqa: F401  (fixture: 45 generated 64 x 64 JPEGs)
from test_gpu_featloss import assert_same_state, build, full_state
from test_gpu_parity import DEV, FIRST_STEP_TOL, oracle_twin_fp64, rel, sync_from_oracle
from test_gpu_siblings import build_vae, sib_inputs

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, os.cpu_count() or 1))

PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
G = importlib.import_module(PKG + ".geometry")
ops = importlib.import_module(PKG + ".ops")
data = importlib.import_module(PKG + ".data")

# ======================================================================================================================
# The kernel against the f64 restatement of its contract
# ======================================================================================================================
# workgroups = partials of a launch: ceil(steps / 256), at most 1024; steps = n / 4 on the 16-byte path, n on the other; the
# one-wave final pass takes 64 partials per turn of its loop, a lane more than one grid-stride step from steps > 262144 on
SHAPES = [(1, 1, 4, 4),             # one vector per row
          (3, 3, 5, 7),             # W % 4 != 0: the one-element-per-lane path, odd everything; 2 workgroups
          (2, 1, 12, 20), (2, 3, 16, 16),
          (5, 3, 64, 64),           # 16-byte path, 60 workgroups: several, still one turn of the final pass
          (24, 3, 64, 64),          # 16-byte path, 288 workgroups: the final pass loops over its partials
          (5, 3, 64, 66),           # one-element path, 248 workgroups: the same there
          (88, 3, 64, 64),          # 16-byte path, 270336 steps: the 1024-workgroup cap, lanes take a second grid-stride step
          (22, 3, 64, 66)]          # one-element path, 278784 steps: the same there
WEIGHTS = [(w, gs) for w in (1.0, 6.0, 0.0, 0.25) for gs in (1.0, 0.37)]     # (w_hole, gscale)


def kernel_inputs(shape):
    g = torch.Generator().manual_seed(100 + sum(shape))
    a, b = torch.rand(shape, generator=g) * 2 - 1, torch.rand(shape, generator=g) * 2 - 1
    a.view(-1)[::7] = b.view(-1)[::7]              # planted: a == b, the gradient there is exactly 0
    return a, b


def near(got, ref, bound, what):
    err = abs(float(got) - ref)
    print(f"{what}: got {float(got):.9g} ref {ref:.9g} err/bound {err / bound if bound else (0.0 if err == 0 else math.inf):.3f}")
    assert math.isfinite(float(got)) and err <= bound, what


def run_kernel(A, Bt, rects, w, gs, loss=True, hole=True, grad=True, stats=None):
    lo = torch.full((1,), 3.0, device=DEV) if loss else None
    ho = torch.full((1,), 3.0, device=DEV) if hole else None
    d = ops.region_mse_forward_backward(A, Bt, rects, w, gs, loss=lo, hole_mse=ho, want_grad=grad, stats=stats)
    assert (d is not None) == grad
    return lo, ho, d


@pytest.mark.parametrize("shape", SHAPES)
def test_region_mse_kernel_vs_f64_restatement(shape):
    """Bounds from the stated arithmetic (U = 2^-24): q = fl(fl(a - b)^2) carries at most (1 + U)^3 - 1 relative error, all
    terms are non-negative, the f64 accumulation and the final rounding to f32 add less than 2 U: loss, hole_mse, S_hole,
    S_valid within 5 U of the restatement; a gradient element within 4 U |g_ref| (the rounding of d, of the coefficient and
    of their product); the counts are equal as integers."""
    Bn, C, H, W = shape
    a, b = kernel_inputs(shape)
    A, Bt = a.to(DEV), b.to(DEV)
    for shift in list(range(0, 8, Bn)) + [None]:                  # None: rects = NULL, no hole anywhere
        rects_h = None if shift is None else PR.offset_rects(Bn, H, W, shift)
        rects = None if rects_h is None else rects_h.to(DEV)
        for w, gs in WEIGHTS:
            ref = PR.region_mse(a, b, rects_h, w)
            gref = PR.region_mse_grad(a, b, rects_h, w, gs)
            what = f"{shape} shift={shift} w={w} gscale={gs}"
            stats = torch.zeros(4, dtype=torch.float64, device=DEV)
            lo, ho, d = run_kernel(A, Bt, rects, w, gs, stats=stats)
            near(lo, ref[0], 5 * U * ref[0], what + " loss")
            near(ho, ref[1], 5 * U * ref[1], what + " hole_mse")
            st = stats.cpu().tolist()
            near(st[0], ref[2], 5 * U * ref[2], what + " S_hole")
            near(st[1], ref[3], 5 * U * ref[3], what + " S_valid")
            assert st[2] == ref[4] and st[3] == ref[5] and st[2] + st[3] == a.numel(), what + " counts"
            if shift is None:
                assert st[0] == 0.0 and st[2] == 0 and float(ho) == 0.0
            gd = d.double().cpu()
            assert bool(torch.isfinite(gd).all()) and bool(((gd - gref).abs() <= 4 * U * gref.abs()).all()), what + " gradient"
            assert float(gd.view(-1)[::7].abs().max()) == 0.0, what + " planted zeros"
            # a second call on the same stats tensor: exactly twice the first (it is always accumulated); everything else:
            # the same bits (written, not accumulated; fixed summation order)
            lo2, ho2, d2 = run_kernel(A, Bt, rects, w, gs, stats=stats)
            assert torch.equal(stats.cpu(), 2 * torch.tensor(st, dtype=torch.float64)), what + " stats accumulate"
            assert torch.equal(lo2, lo) and torch.equal(ho2, ho) and torch.equal(d2, d), what + " run to run"
            # every output alone, the others NULL: the same bits
            l3, _, _ = run_kernel(A, Bt, rects, w, gs, hole=False, grad=False)
            _, h3, _ = run_kernel(A, Bt, rects, w, gs, loss=False, grad=False)
            _, _, d3 = run_kernel(A, Bt, rects, w, gs, loss=False, hole=False)
            s3 = torch.zeros(4, dtype=torch.float64, device=DEV)
            run_kernel(A, Bt, rects, w, gs, loss=False, hole=False, grad=False, stats=s3)
            assert torch.equal(l3, lo) and torch.equal(h3, ho) and torch.equal(d3, d) and s3.cpu().tolist() == st, what + " NULL outputs"


@pytest.mark.parametrize("shape", [(5, 3, 64, 64), (24, 3, 64, 64), (5, 3, 64, 66), (88, 3, 64, 64)])
def test_region_mse_replayed_from_a_graph_equals_the_eager_launch_bitwise(shape):
    a, b = kernel_inputs(shape)
    A, Bt, rects = a.to(DEV), b.to(DEV), PR.cycle_rects(*shape[:1], *shape[2:]).to(DEV)
    se = torch.zeros(4, dtype=torch.float64, device=DEV)
    lo_e, ho_e, d_e = run_kernel(A, Bt, rects, 6.0, 0.37, stats=se)                   # also sizes the workspace
    lo, ho = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    st = torch.zeros(4, dtype=torch.float64, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):                                       # one stream, no parallel branches
            d = ops.region_mse_forward_backward(A, Bt, rects, 6.0, 0.37, loss=lo, hole_mse=ho, want_grad=True, stats=st)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        d.zero_(), lo.zero_(), ho.zero_(), st.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(lo, lo_e) and torch.equal(ho, ho_e) and torch.equal(d, d_e) and torch.equal(st, se)
    Bt.copy_(A)                                                                   # the graph reads its inputs at replay time
    g.replay()
    torch.cuda.synchronize()
    assert float(lo) == 0.0 and float(ho) == 0.0 and float(d.abs().max()) == 0.0


def test_region_mse_wrapper_rejects_mismatched_tensors():
    a = torch.zeros(2, 3, 8, 8, device=DEV)
    loss = torch.zeros(1, device=DEV)
    f = ops.region_mse_forward_backward
    for bad in (dict(b=torch.zeros(2, 3, 8, 4, device=DEV)), dict(b=a.double()), dict(rects=torch.zeros(3, 8, device=DEV)),
                dict(rects=torch.zeros(2, 8, device=DEV, dtype=torch.float64)), dict(rects=torch.zeros(2, 8)),
                dict(rects=torch.zeros(2, 16, device=DEV)[:, ::2]), dict(stats=torch.zeros(4, device=DEV)),
                dict(stats=torch.zeros(3, dtype=torch.float64, device=DEV)), dict(w_hole=-1.0), dict(w_hole=float("nan")),
                dict(loss=None)):
        kw = dict(a=a, b=a, rects=None, w_hole=1.0, gscale=1.0, loss=loss)
        kw.update(bad)
        with pytest.raises(RuntimeError, match="region_mse_forward_backward|contiguous|cuda"):
            f(**kw)
    with pytest.raises(RuntimeError):
        f(a.view(6, 8, 8), a.view(6, 8, 8), None, 1.0, 1.0, loss=loss)


# ======================================================================================================================
# The kernel's mask is the degradation kernel's rectangle; want_rects and bind_noisy
# ======================================================================================================================
def test_the_mask_is_the_degrade_kernels_rectangle_and_the_loader_hands_it_out(jpeg_folder):  # noqa: F811
    ds = data.ResidentImages.from_folder(jpeg_folder, device=DEV, workers=1)
    idx = torch.arange(len(ds))
    dg = data.Degrade(0.0, rect=True)
    loader = data.DeviceLoader(ds, idx, 8, shuffle=True, degrade=dg)
    loader.want_rects(True)
    torch.manual_seed(42)
    unbound, n_hole_sum = [], 0
    bounds = list(loader.global_batches(len(ds)))
    for k, (noisy, clean) in enumerate(loader):
        b = clean.shape[0]
        rects = loader.last_rects
        assert rects.dtype == torch.float32 and tuple(rects.shape) == (b, 8) and rects.is_cuda
        want = ops.degrade_params(loader.last_base_seed, bounds[k][0], b, 0.0, True, 64, 64, data.degrade_bounds(64, 64), DEV)
        assert torch.equal(rects, want)
        stats = torch.zeros(4, dtype=torch.float64, device=DEV)
        ops.region_mse_forward_backward(noisy, clean, rects, 1.0, 1.0, stats=stats)
        s_hole, s_valid, n_hole, n_valid = stats.cpu().tolist()
        r = rects.cpu().double()
        assert s_valid == 0.0, "without noise the pair differs inside the rectangle only: the two kernels agree on it"
        assert n_hole == float((3 * r[:, 2] * r[:, 3]).sum()) and n_hole + n_valid == clean.numel() and s_hole > 0
        assert bool((PR.region_mask(rects, *clean.shape) | (noisy.cpu() == clean.cpu())).all())
        n_hole_sum += n_hole
        unbound.append((noisy.cpu(), clean.cpu()))
    assert len(unbound) == 6 and n_hole_sum > 0
    # rect=False: the geometry entries are 0 -- no hole
    flat = data.DeviceLoader(ds, idx, 45, shuffle=False, degrade=data.Degrade(0.25, rect=False))
    flat.want_rects(True)
    (noisy, clean), = list(flat)
    assert float(flat.last_rects[:, 2:6].abs().max()) == 0.0 and float(flat.last_rects[:, 1].max()) > 0
    stats = torch.zeros(4, dtype=torch.float64, device=DEV)
    ops.region_mse_forward_backward(noisy, clean, flat.last_rects, 1.0, 1.0, stats=stats)
    assert stats.cpu().tolist()[2] == 0.0
    flat.want_rects(False)
    assert flat.last_rects is None
    # bind_noisy: full batches are assembled in the bound tensor, the same bytes; the ragged last batch gets its own
    out_n, out_c = torch.empty(8, 3, 64, 64, device=DEV), torch.empty(8, 3, 64, 64, device=DEV)
    loader.bind_noisy(out_n), loader.bind_output(out_c)
    torch.manual_seed(42)
    for k, (noisy, clean) in enumerate(loader):
        if clean.shape[0] == 8:
            assert noisy.data_ptr() == out_n.data_ptr() and clean.data_ptr() == out_c.data_ptr()
        else:
            assert k == 5 and noisy.shape[0] == 5 and noisy.data_ptr() != out_n.data_ptr()
        assert torch.equal(noisy.cpu(), unbound[k][0]) and torch.equal(clean.cpu(), unbound[k][1])
    loader.bind_noisy(None)
    torch.manual_seed(42)
    assert next(iter(loader))[0].data_ptr() != out_n.data_ptr()


# ======================================================================================================================
# Paired with nothing to pair is the unpaired step; off means off
# ======================================================================================================================
@pytest.mark.parametrize("graphed", [False, True])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_paired_step_with_nothing_to_pair_is_bitwise_the_unpaired_step(dtype, graphed):
    """noisy = real.clone(), hole_weight = 1: the Encoder's input conversion and the noisy real batch come from two launches
    instead of the merged one (documented bit-identical), everything else is the same launch sequence."""
    res = []
    for paired in (False, True):
        e, g, d, tr = build(64, dtype=dtype)
        fn = tr.train_step_graphed if graphed else tr.train_step
        losses = []
        for step in range(3):
            real, ez, er, ec = (t.to(DEV) for t in make_inputs(4, 64, 7064 + step))
            kw = dict(noisy=real.clone()) if paired else {}
            losses.append(fn(real, 60, ez, er, ec, **kw).cpu().clone())
        res.append((losses, full_state(e, g, d, tr)))
        if graphed:
            assert tr._graph is not None and (tr.graph_noisy_input() is not None) == paired
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(a, b) and float(b[7]) == 0.0
    assert_same_state(res[0][1], res[1][1])


def test_hole_weight_without_the_keywords_changes_nothing():
    res = []
    for kw in ({}, dict(hole_weight=6.0)):
        e, g, d, tr = build(64, **kw)
        n0 = ops.launch_count()
        losses = []
        for step in range(2):
            real, ez, er, ec = (t.to(DEV) for t in make_inputs(4, 64, 7064 + step))
            losses.append(tr.train_step(real, 60, ez, er, ec).cpu().clone())
        res.append((losses, full_state(e, g, d, tr), ops.launch_count() - n0))
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(a, b) and float(b[7]) == 0.0
    assert_same_state(res[0][1], res[1][1])
    assert res[0][2] == res[1][2], "hole_weight, with no pair given, changed the number of kernel launches"
    assert "hole_mse" not in tr.loss_dict() and tr.hole_weight == 6.0      # reported only after a step that used the term
    real, ez, er, ec = (t.to(DEV) for t in make_inputs(4, 64, 7070))
    assert "hole_mse" not in tr.loss_dict(tr.train_step(real, 60, ez, er, ec, noisy=real.clone()))     # paired, no rects
    assert tr.loss_dict(tr.train_step(real, 60, ez, er, ec, noisy=real.clone(), rects=PR.hand_rects(4).to(DEV)))["hole_mse"] > 0
    assert "hole_mse" not in tr.loss_dict(tr.train_step(real, 60, ez, er, ec))


# ======================================================================================================================
# The first paired step against ref_step
# ======================================================================================================================
_REF, _RUN = {}, {}
NOISY_SEED = PR.NOISY_SEED


def pair_inputs(B=4, S=64, seed=7064):
    real, ez, er, ec = make_inputs(B, S, seed)
    rects = PR.hand_rects(B)
    return real, PR.make_noisy(real, rects, NOISY_SEED), ez, er, ec, rects


def ref_first_step(hw):
    if hw not in _REF:
        real, noisy, ez, er, ec, rects = pair_inputs()
        _REF[hw] = PR.ref_step(R.RefVAEGAN(img_size=64, seed=42), real, noisy, ez, er, ec, 60, rects=rects, hole_weight=hw)
    return _REF[hw]


def hip_first_step(hw, with_nhwc=False):
    """(loss dict, loss vector, full state) of the first paired iteration from the seed-42 state, once per variant."""
    key = (hw, with_nhwc)
    if key not in _RUN:
        e, g, d, tr = build(64, hole_weight=hw)
        real, noisy, ez, er, ec, rects = (t.to(DEV) for t in pair_inputs())
        nhwc = ops.nchw_to_nhwc(noisy, G.padc(3, tr.dt), tr.dt) if with_nhwc else None
        vec = tr.train_step(real, 60, ez, er, ec, noisy=noisy, noisy_nhwc=nhwc, rects=rects)
        _RUN[key] = (tr.loss_dict(vec, 60), vec.cpu().clone(), full_state(e, g, d, tr))
    return _RUN[key]


@pytest.mark.parametrize("hw", [1.0, 6.0])
def test_first_paired_step_vs_ref_step(hw):
    """Every loss within FIRST_STEP_TOL of tests/test_gpu_parity.py; hole_mse is a pure forward quantity of the initial
    weights like recon_loss and takes its 1e-4."""
    ref = ref_first_step(hw)
    got, vec, state = hip_first_step(hw)
    tol = dict(FIRST_STEP_TOL)
    if hw != 1.0:
        tol["hole_mse"] = FIRST_STEP_TOL["recon_loss"]
    print({k: f"{got[k]:.6g} / {ref[k]:.6g} ({rel(got[k], ref[k]):.1e})" for k in tol})
    assert sorted(got) == sorted(tol) == sorted(ref)
    for k, t in tol.items():
        assert rel(got[k], ref[k]) <= t, f"hole_weight={hw} {k}: hip {got[k]} ref_step {ref[k]}"
    assert (float(vec[7]) > 0) == (hw != 1.0) and float(vec[0]) == got["recon_loss"]
    # the loader's NHWC copy of `noisy` in place of the conversion: the same bits
    got_n, vec_n, state_n = hip_first_step(hw, with_nhwc=True)
    assert torch.equal(vec, vec_n) and got == got_n
    assert_same_state(state, state_n)


def test_paired_step_rejects_a_wrong_nhwc_tensor_or_rects():
    e, g, d, tr = build(64, hole_weight=6.0)
    real, noisy, ez, er, ec, rects = (t.to(DEV) for t in pair_inputs())
    good = ops.nchw_to_nhwc(noisy, G.padc(3, tr.dt), tr.dt)
    before = full_state(e, g, d, tr)
    for bad in (dict(noisy_nhwc=good[:2]), dict(noisy_nhwc=good.bfloat16()), dict(noisy_nhwc=good.cpu()),
                dict(rects=rects[:2]), dict(rects=rects.double()), dict(noisy=noisy[:, :, :32]), dict(noisy=noisy.cpu())):
        kw = dict(noisy=noisy, rects=rects)
        kw.update(bad)
        with pytest.raises(RuntimeError):
            tr.train_step(real, 60, ez, er, ec, **kw)
    assert_same_state(before, full_state(e, g, d, tr))


def test_the_weight_moves_the_encoder_and_the_generator_and_leaves_the_discriminator():
    """The Discriminator's two updates precede the term: from one state, hole_weight 6 and 1 leave it bitwise identical."""
    s1, s6 = hip_first_step(1.0)[2], hip_first_step(6.0)[2]
    differs = {"E": False, "G": False}
    for k in s1:
        if k.startswith("D.") or k.startswith("opt_D."):
            assert torch.equal(s1[k], s6[k]), k
        elif k.startswith("opt_E.exp_avg") or k.startswith("opt_G.exp_avg"):
            differs[k[4]] |= not torch.equal(s1[k], s6[k])
    assert differs == {"E": True, "G": True}


def test_weighted_gradient_path_in_isolation_vs_fp64_ref_step():
    """epoch = 0 (KL weight 0), alpha_adv = 0, hole_weight = 6: every gradient that reaches the Generator and the Encoder is
    the region-weighted term's, from the kernel's d_recon.  Teacher-forced from the oracle's state, lr = 0 on both sides,
    gradient = exp_avg / (1 - beta1) after the first Adam step; bound per tensor as
    tests/test_gpu_featloss.test_feature_gradient_path_in_isolation_vs_fp64_ref_step: max error relative to the tensor's max
    <= max(1e-5, 4 x the CPU-fp32 ref_step's own error against the fp64 one)."""
    S, B = 64, 4
    e, g, d, tr = build(S, lr=0.0, alpha_adv=0.0, hole_weight=6.0)
    o = R.RefVAEGAN(img_size=S, seed=42, lr=0.0)
    sync_from_oracle(o, e, g, d, tr)
    o64 = oracle_twin_fp64(o)
    real, ez, er, ec = make_inputs(B, S, SR.ISO_SEED)
    rects = PR.hand_rects(B)
    noisy = PR.make_noisy(real, rects, PR.ISO_NOISY_SEED)        # every pre-activation of the fp64 forward >= 2e-6 from its kink
    kw = dict(rects=rects, hole_weight=6.0, alpha_adv=0.0)
    PR.ref_step(o64, real, noisy, ez, er, ec, 0, **kw)
    PR.ref_step(o, real, noisy, ez, er, ec, 0, **kw)
    tr.train_step(real.to(DEV), 0, ez.to(DEV), er.to(DEV), ec.to(DEV), noisy=noisy.to(DEV), rects=rects.to(DEV))
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
# Graph replay and the capture key
# ======================================================================================================================
def test_graphed_paired_step_equals_eager_static_inputs_and_recapture():
    B, S = 4, 64
    (ee, ge, de, te), (eg, gg, dg, tg) = (build(S, hole_weight=6.0) for _ in range(2))

    def batch(step):
        real, ez, er, ec = make_inputs(B, S, 7064 + step)
        rects = PR.offset_rects(B, S, S, step)
        return [t.to(DEV) for t in (real, ez, er, ec, PR.make_noisy(real, rects, 20 + step), rects)]

    def both(step, direct=False):
        real, ez, er, ec, noisy, rects = batch(step)
        le = te.train_step(real, 60, ez, er, ec, noisy=noisy, rects=rects).cpu().clone()
        if direct:                      # the batch written straight into the static buffers: no copy on the way in
            gi, gn, gr = tg.graph_input(), tg.graph_noisy_input(), tg.graph_rects_input()
            gi.copy_(real), gn.copy_(noisy), gr.copy_(rects)
            real, noisy, rects = gi, gn, gr
        lg = tg.train_step_graphed(real, 60, ez, er, ec, noisy=noisy, rects=rects).cpu().clone()
        assert torch.equal(le, lg), (step, le, lg)
        assert float(le[7]) > 0
        return le

    for step in range(3):
        both(step)
    assert_same_state(full_state(ee, ge, de, te), full_state(eg, gg, dg, tg))
    graph1 = tg._graph
    assert graph1 is not None and len(graph1[1]) == 1            # eager, capture + replay, replay: ONE graph
    assert tuple(tg.graph_noisy_input().shape) == (B, 3, S, S) and tuple(tg.graph_rects_input().shape) == (B, 8)
    for step in range(3, 5):
        both(step, direct=True)
    assert tg._graph is graph1
    assert_same_state(full_state(ee, ge, de, te), full_state(eg, gg, dg, tg))
    assert "hole_mse" in tg.loss_dict() and tg.loss_dict() == te.loss_dict()
    # a replay validates what it copies into its static buffers: copy_ would convert a dtype or broadcast a row silently
    real, ez, er, ec, noisy, rects = batch(5)
    before = full_state(eg, gg, dg, tg)
    for bad in (dict(noisy=noisy.double()), dict(noisy=noisy[:1]), dict(noisy=noisy.cpu()), dict(rects=rects[:1]),
                dict(rects=rects.double()), dict(rects=rects.cpu())):
        kw = dict(noisy=noisy, rects=rects)
        kw.update(bad)
        with pytest.raises(RuntimeError):
            tg.train_step_graphed(real, 60, ez, er, ec, **kw)
    assert tg._graph is graph1
    assert_same_state(before, full_state(eg, gg, dg, tg))
    # a new weight: the next call may not replay the old graph (the scalar is frozen in it)
    te.hole_weight = tg.hole_weight = 2.5
    for step in range(5, 8):
        both(step)
    assert tg._graph is not graph1 and tg._graph.key != graph1.key
    assert_same_state(full_state(ee, ge, de, te), full_state(eg, gg, dg, tg))
    graph2 = tg._graph
    # without rects: another capture again (the MSE launches of the unpaired step), slot 7 reads 0
    real, ez, er, ec, noisy, rects = batch(8)
    for _ in range(2):
        out = tg.train_step_graphed(real, 60, ez, er, ec, noisy=noisy)
    assert tg._graph is not graph2 and tg.graph_rects_input() is None and float(out[7]) == 0.0


# ======================================================================================================================
# VAETrainer
# ======================================================================================================================
def build_vae_hw(S, hw):
    e, g, tr = build_vae(S)
    tr.hole_weight = hw
    return e, g, tr


def vae_state(e, g, tr):
    torch.cuda.synchronize()
    out = {f"{n}.{k}": v.cpu().clone() for n, m in (("E", e), ("G", g)) for k, v in m.state_dict().items()}
    for a in ("flat_p", "exp_avg", "exp_avg_sq", "state_dev"):
        out["opt." + a] = getattr(tr.opt, a).cpu().clone()
    return out


def test_vae_paired_step_vs_ref_vae_step():
    """tests/test_gpu_siblings.check_vae's first-step bound (1e-4: pure forward passes of the initial weights)."""
    S, B = 64, 4
    img, _, eps_z, _ = sib_inputs(B, S, 0)
    rects = PR.hand_rects(B)
    noisy = PR.make_noisy(img, rects, NOISY_SEED)
    for hw, slots in ((1.0, 4), (6.0, 5)):
        ref = PR.ref_vae_step(SIB.RefVAE(img_size=S, seed=42), img, noisy, eps_z, 25, rects=rects, hole_weight=hw)
        e, g, tr = build_vae_hw(S, hw)
        vec = tr.train_step(img.to(DEV), None, eps_z.to(DEV), epoch=25, noisy=noisy.to(DEV), rects=rects.to(DEV)).cpu()
        assert vec.numel() == slots
        got = dict(zip(("recon_loss", "kl_loss", "total"), vec[:3].tolist()))
        if hw != 1.0:
            got["hole_mse"] = float(vec[4])
        print(hw, {k: f"{got[k]:.6g} / {ref[k]:.6g} ({rel(got[k], ref[k]):.1e})" for k in ref})
        assert sorted(got) == sorted(ref)
        for k in ref:
            assert rel(got[k], ref[k]) <= 1e-4, f"hole_weight={hw} {k}: hip {got[k]} ref_vae_step {ref[k]}"
    # the term off (no rects): 4 slots whatever the weight
    e, g, tr = build_vae_hw(S, 6.0)
    assert tr.train_step(img.to(DEV), None, eps_z.to(DEV), epoch=25, noisy=noisy.to(DEV)).numel() == 4


def test_vae_paired_with_the_callers_own_noisy_is_bitwise_the_unpaired_step():
    S, B = 64, 4
    res = []
    for paired in (False, True):
        e, g, tr = build_vae(S)
        out = []
        for step in range(2):
            img, eps_img, eps_z, _ = (t.to(DEV) if torch.is_tensor(t) else t for t in sib_inputs(B, S, step))
            if paired:
                # clamp(img + sigma * eps_img, -1, 1) as the unpaired step forms it, handed over as `noisy`
                _, noisy = ops.noisy_clamp_to_nhwc(img, eps_img, tr.sigma, G.padc(3, tr.dt), tr.dt)
                out.append(tr.train_step(img, None, eps_z, epoch=25, noisy=noisy).cpu().clone())
            else:
                out.append(tr.train_step(img, eps_img, eps_z, epoch=25).cpu().clone())
        res.append((out, vae_state(e, g, tr)))
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(a, b)
    assert_same_state(res[0][1], res[1][1])


def test_vae_paired_step_graphed_equals_eager():
    S, B = 64, 4
    res = []
    for graphed in (False, True):
        e, g, tr = build_vae_hw(S, 6.0)
        out = []
        for step in range(3):
            img, _, eps_z, _ = sib_inputs(B, S, step)
            rects = PR.hand_rects(B)
            noisy = PR.make_noisy(img, rects, 30 + step)
            img, eps_z, noisy, rects = (t.to(DEV) for t in (img, eps_z, noisy, rects))
            if graphed:
                out.append(tr.step_graphed(img, None, eps_z, noisy=noisy, rects=rects, epoch=25).cpu().clone())
            else:
                out.append(tr.train_step(img, None, eps_z, epoch=25, noisy=noisy, rects=rects).cpu().clone())
        if graphed:
            assert tr._gstate is not None and len(tr._gstate.sin) == 4
        res.append((out, vae_state(e, g, tr)))
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(a, b) and a.numel() == 5 and float(a[4]) > 0
    assert_same_state(res[0][1], res[1][1])


# ======================================================================================================================
# paired_test_epoch(regions=True)
# ======================================================================================================================
OLD_KEYS = {"test_loss", "recon_loss", "kl_loss", "ssim", "psnr", "ssim_noisy", "psnr_noisy", "samples", "batches"}
REGION_KEYS = {k + s for k in ("mse_hole", "mse_valid", "psnr_hole", "psnr_valid", "hole_fraction") for s in ("", "_noisy")}


def test_paired_test_epoch_regions_vs_cpu_restatement_on_the_oracle_nets(jpeg_folder):  # noqa: F811
    """Set up as tests/test_gpu_degrade.test_paired_test_epoch_vs_cpu_restatement_on_the_oracle_nets, with its tolerances
    for what it checks (test_loss 1e-4 relative, PSNR 1e-3 dB); the region MSEs of the reconstruction take the 1e-4 relative
    that test holds the squared-error sum to, those of the input (the same bytes on both sides) the kernel test's 5 U."""
    S = 64
    ds = data.ResidentImages.from_folder(jpeg_folder, device=DEV, workers=1)
    loader = data.DeviceLoader(ds, torch.arange(40, 45), 2, shuffle=False, degrade=data.Degrade(0.25))
    loader.want_rects(True)
    torch.manual_seed(5)
    pairs = [(n.cpu(), c.cpu(), loader.last_rects.cpu()) for n, c in loader]   # 5 images: 2 + 2 + 1
    loader.want_rects(False)
    e, g, d, tr = build(S)
    o = R.RefVAEGAN(img_size=S, seed=42)
    real, ez, er, ec = make_inputs(4, S, 4711)
    o.train_step(real, ez, er, ec, 60)                                         # non-trivial BatchNorm running statistics
    sync_from_oracle(o, e, g, d, tr)
    gen = torch.Generator().manual_seed(99)
    eps = [torch.randn(c.shape[0], 100, generator=gen) for _, c, _ in pairs]
    batches, tot, seen = [], 0.0, 0
    with torch.no_grad():
        for (noisy, clean, rects), eps_z in zip(pairs, eps):
            mu, logvar = R.encoder_forward(o.E, noisy, False)
            logvar = torch.clamp(logvar, min=-10, max=10)
            z = (mu + torch.exp(0.5 * logvar) * eps_z).unsqueeze(-1).unsqueeze(-1)
            recon = R.generator_forward(o.G, o.g_spec, z, False)
            tot += float(torch.nn.functional.mse_loss(recon, clean, reduction="sum") + R.kl_sum(mu, logvar))
            seen += clean.shape[0]
            batches.append((recon, noisy, clean, rects))
    want = PR.ref_paired_regions(batches)
    noise_fn = lambda i, noisy: eps[i].to(DEV)                                  # noqa: E731
    torch.manual_seed(5)                                                        # the same epoch seed -> the same pairs
    got = V.paired_test_epoch(e, g, loader, noise_fn=noise_fn, regions=True)
    print("regions", {k: got[k] for k in sorted(REGION_KEYS)}, "restatement", want)
    assert set(got) == OLD_KEYS | REGION_KEYS and set(want) == REGION_KEYS
    assert loader._rects is False and loader.last_rects is None and loader._nhwc is None   # both requests are withdrawn
    assert abs(got["test_loss"] - tot / seen) <= 1e-4 * abs(tot / seen)
    assert 0 < want["hole_fraction"] < 1 / 16 and got["hole_fraction"] == want["hole_fraction"] == got["hole_fraction_noisy"]
    for k in ("mse_hole", "mse_valid"):
        assert rel(got[k], want[k]) <= 1e-4, k
        assert rel(got[k + "_noisy"], want[k + "_noisy"]) <= 5 * U, k
    for k in ("psnr_hole", "psnr_valid", "psnr_hole_noisy", "psnr_valid_noisy"):
        assert abs(got[k] - want[k]) < 1e-3, k
    # the two regions add up to the whole image: recon_loss is the f32-accumulated mean of the batch MSEs (weights b; three
    # batches of 2, 2, 1), each a rounded f32: a few U
    f = got["hole_fraction"]
    assert rel(f * got["mse_hole"] + (1 - f) * got["mse_valid"], got["recon_loss"]) <= 16 * U
    # regions=False: exactly the old keys, the old numbers
    torch.manual_seed(5)
    old = V.paired_test_epoch(e, g, loader, noise_fn=noise_fn)
    assert set(old) == OLD_KEYS and all(old[k] == got[k] for k in OLD_KEYS)
    # a loader that was handing out rectangles before the pass still does afterwards
    loader.want_rects(True)
    torch.manual_seed(5)
    V.paired_test_epoch(e, g, loader, noise_fn=noise_fn, regions=True)
    assert loader._rects is True
    # rect=False: no hole anywhere
    flat = data.DeviceLoader(ds, torch.arange(40, 45), 2, shuffle=False, degrade=data.Degrade(0.25, rect=False))
    torch.manual_seed(5)
    nf = V.paired_test_epoch(e, g, flat, noise_fn=noise_fn, regions=True)
    assert nf["hole_fraction"] == 0.0 and nf["psnr_hole"] == math.inf and nf["mse_hole"] == 0.0
    assert nf["hole_fraction_noisy"] == 0.0 and nf["psnr_hole_noisy"] == math.inf
    assert rel(nf["mse_valid"], nf["recon_loss"]) <= 16 * U and math.isfinite(nf["psnr_valid"])
    # a plain iterable knows no rectangles
    with pytest.raises(RuntimeError, match="regions=True"):
        V.paired_test_epoch(e, g, [(n.to(DEV), c.to(DEV)) for n, c, _ in pairs], noise_fn=noise_fn, regions=True)


# ======================================================================================================================
# bf16
# ======================================================================================================================
def test_bf16_first_paired_step_with_the_weight_on():
    """S = 64, B = 8, hole_weight = 6, bf16 engine, against the f64 ref_step with the project's stated bf16 loss bound (3e-2:
    bf16 keeps 8 significant bits; tests/test_gpu_featloss.test_bf16_first_step_feature_loss and
    tests/test_gpu_parity.test_bf16_engine_tracks_fp32_oracle hold the first-iteration losses to it)."""
    S, B = 64, 8
    real, noisy, ez, er, ec, rects = pair_inputs(B)
    ref = PR.ref_step(R.RefVAEGAN(img_size=S, seed=42).double_(), real, noisy, ez, er, ec, 60, rects=rects, hole_weight=6.0)
    e, g, d, tr = build(S, dtype="bf16", hole_weight=6.0)
    got = tr.loss_dict(tr.train_step(real.to(DEV), 60, ez.to(DEV), er.to(DEV), ec.to(DEV), noisy=noisy.to(DEV),
                                     rects=rects.to(DEV)), 60)
    print({k: f"{got[k]:.6g} / {ref[k]:.6g} ({rel(got[k], ref[k]):.1e})" for k in ref})
    for k in V.LOSS_NAMES + ("hole_mse",):
        assert rel(got[k], ref[k]) <= 3e-2, f"bf16 {k}: hip {got[k]} ref_step {ref[k]}"
