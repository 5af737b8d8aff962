"""GPU: the Discriminator-feature reconstruction loss (Larsen et al. 2016, eq. 2) from the kernel up to the trainer:
vg_feat_mse_forward_backward against the f64 restatement of its contract, Discriminator.features against the oracle's
prefix forward, and the iteration with the feature on against tests/_featloss_ref.ref_step (the oracle's iteration with
the block added) -- losses, BatchNorm counters, the gradient path in isolation, hipGraph replay and the capture key."""
import importlib
import os

import numpy as np
import pytest
import torch

import _featloss_ref as FR
import vaegan_ref as R
from _featloss_ref import U, UB
from _inputs import make_inputs

import vaegan_amd as V
from test_gpu_parity import DEV, FIRST_STEP_TOL, _LocalReducer, oracle_twin_fp64, rel, sync_from_oracle

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, os.cpu_count() or 1))

PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
G = importlib.import_module(PKG + ".geometry")
ops = importlib.import_module(PKG + ".ops")
TDT = {G.F32: torch.float32, G.BF16: torch.bfloat16}


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


def full_state(e, g, d, tr):
    """Every parameter, buffer and Adam moment (+ step counters) on the host."""
    torch.cuda.synchronize()
    out = {}
    for n, m in (("E", e), ("G", g), ("D", d)):
        for k, v in m.state_dict().items():
            out[f"{n}.{k}"] = v.cpu().clone()
    for n, o in (("E", tr.opt_E), ("G", tr.opt_G), ("D", tr.opt_D)):
        for a in ("flat_p", "exp_avg", "exp_avg_sq", "state_dev"):
            out[f"opt_{n}.{a}"] = getattr(o, a).cpu().clone()
        out[f"opt_{n}.steps"] = torch.tensor(o.steps)
    return out


def assert_same_state(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ======================================================================================================================
# The kernel against the f64 restatement of its contract
# ======================================================================================================================
FEAT_SIZES = [8,                                  # one 16-byte vector of bf16, two of f32
              8 * 1001,                           # more than one workgroup, the last one not full
              1 * 4 * 4 * 512, 4 * 8 * 8 * 256, 2 * 16 * 16 * 128,      # stages 3, 2, 1 at S = 64
              8 * (1024 * 256 + 300)]             # more vectors than 1024 workgroups x 256 threads: the grid-stride loop


def feat_inputs(n, dtype):
    """Values exactly representable in the storage type, as f64."""
    g = torch.Generator().manual_seed(n + dtype)
    return [(torch.randn(n, generator=g) * s).to(TDT[dtype]).double() for s in (1.0, 1.0, 1e-3)]


def check(got, ref, bound, what, bf16=False):
    got = got.detach().double().cpu().reshape(ref.shape)
    bound = torch.as_tensor(bound, dtype=torch.float64).expand(ref.shape).clone()
    if bf16:
        bound = bound + UB * (ref.abs() + bound)        # half a bf16 ulp of the result (UB = 2^-8)
    err = (got - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: max err {float(err.max()):.3e}, max err/bound {ratio:.3f}")
    assert bool(torch.isfinite(got).all()), what
    assert bool((err <= bound).all()), f"{what}: max err/bound {ratio:.3f}"


@pytest.mark.parametrize("dtype", [G.F32, G.BF16])
@pytest.mark.parametrize("n", FEAT_SIZES)
def test_feat_mse_kernel_vs_f64_restatement(n, dtype):
    a, b, d0 = feat_inputs(n, dtype)
    A, Bt, D0 = (t.to(TDT[dtype]).to(DEV) for t in (a, b, d0))
    ref = FR.feat_mse(a, b)
    # loss, in the accumulation model of tests/test_gpu_pointwise.py ("f64 sums of f32 terms"): term = (a - b)^2 in f32 is
    # the difference (1 rounding, doubled by the square) and the square (1 rounding): 3 U relative; the terms are summed in
    # f64; each workgroup's partial is stored as f32 (U), the f64 sum of the partials / n is rounded to f32 (U): 5 U |ref|.
    lbound = 5 * U * ref
    for gscale in (1.0, 0.37):
        loss = torch.full((1,), 3.0, device=DEV)
        d = D0.clone()
        assert ops.feat_mse_forward_backward(A, Bt, d, gscale, loss, False, dtype) is d
        check(loss, ref.view(1), lbound, f"loss n={n}")
        # gradient: g = f32(gscale 2 / n) (a - b): the coefficient (U) and the difference (U); g is then added onto d with at
        # most one more rounding of g (none where the compiler contracts to an fma) and one rounding of the sum in f32:
        # 3 U |g| + U |d + g|; bf16 storage: + half a bf16 ulp of the result
        gref, dref = FR.feat_mse_grad_add(a, b, d0, gscale)
        check(d, dref, 3 * U * gref.abs() + U * dref.abs(), f"d_inout n={n} gscale={gscale}", dtype == G.BF16)
        # d_inout = NULL: the same loss bits, nothing else written; accumulate: the slot's value + the loss, one more rounding
        loss2 = torch.full((1,), 3.0, device=DEV)
        assert ops.feat_mse_forward_backward(A, Bt, None, gscale, loss2, False, dtype) is None
        assert torch.equal(loss2, loss)
        for dd in (None, D0.clone()):
            acc = torch.full((1,), 3.0, device=DEV)
            ops.feat_mse_forward_backward(A, Bt, dd, gscale, acc, True, dtype)
            check(acc, (3.0 + ref).view(1), lbound + U * (3.0 + ref), f"accumulated loss n={n}")
            assert float(acc) == float(torch.tensor(3.0) + loss.cpu()[0]), "accumulate is slot + the very same loss, in f32"
            if dd is not None:
                assert torch.equal(dd, d), "accumulate_loss must not change the gradient"
        # run to run: the same bits
        loss3, d3 = torch.zeros(1, device=DEV), D0.clone()
        ops.feat_mse_forward_backward(A, Bt, d3, gscale, loss3, False, dtype)
        assert torch.equal(loss3, loss) and torch.equal(d3, d)


@pytest.mark.parametrize("dtype", [G.F32, G.BF16])
def test_feat_mse_launch_is_capturable_in_a_graph(dtype):
    n = 4 * 8 * 8 * 256
    a, b, d0 = feat_inputs(n, dtype)
    A, Bt, D0 = (t.to(TDT[dtype]).to(DEV) for t in (a, b, d0))
    loss_e, d_e = torch.zeros(1, device=DEV), D0.clone()
    ops.feat_mse_forward_backward(A, Bt, d_e, 0.37, loss_e, False, dtype)        # also sizes the workspace
    loss, d = torch.zeros(1, device=DEV), D0.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):                                       # one stream, no parallel branches
            ops.feat_mse_forward_backward(A, Bt, d, 0.37, loss, False, dtype)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        d.copy_(D0), loss.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss, loss_e) and torch.equal(d, d_e)
    Bt.copy_(A)                                                                   # the graph reads its inputs at replay time
    d.copy_(D0)
    g.replay()
    torch.cuda.synchronize()
    assert float(loss) == 0.0 and torch.equal(d, D0)


def test_feat_mse_wrapper_rejects_mismatched_tensors():
    a = torch.zeros(64, device=DEV)
    loss = torch.zeros(1, device=DEV)
    with pytest.raises(RuntimeError):
        ops.feat_mse_forward_backward(a, a.bfloat16(), None, 1.0, loss, False, G.F32)
    with pytest.raises(RuntimeError):
        ops.feat_mse_forward_backward(a, torch.zeros(32, device=DEV), None, 1.0, loss, False, G.F32)
    with pytest.raises(RuntimeError):
        ops.feat_mse_forward_backward(a, a, torch.zeros(32, device=DEV), 1.0, loss, False, G.F32)
    with pytest.raises(RuntimeError):
        ops.feat_mse_forward_backward(a.cpu(), a.cpu(), None, 1.0, loss, False, G.F32)


# ======================================================================================================================
# Discriminator.features
# ======================================================================================================================
def test_features_accessor_vs_oracle_prefix_forward():
    """S = 64, B = 4, fp32, eval then train, every valid stage; the project's forward known-answer tolerance
    (tests/test_gpu_parity.py, the Encoder forward test): rtol 1e-4 / atol 2e-5."""
    S, B = 64, 4
    e, g, d, tr = build(S)
    o = R.RefVAEGAN(img_size=S, seed=42)
    x = make_inputs(B, S, 1000 + S)[0]
    assert d.feature_layers() == FR.feature_stages(o.d_spec) == [1, 2, 3]
    for train in (False, True):
        d.train(train)
        for l in (1, 2, 3):
            with torch.no_grad():
                _, ref = FR.d_forward_tapped(o.D, o.d_spec, x, l, train)
            xg = x.to(DEV).requires_grad_(True)          # no autograd whatever the input asks for
            f = d.features(xg, l)
            assert f.dtype == torch.float32 and f.shape == ref.shape == (B, 64 << l, 32 >> l, 32 >> l) and not f.requires_grad
            np.testing.assert_allclose(f.cpu().numpy(), ref.numpy(), rtol=1e-4, atol=2e-5, err_msg=f"train={train} l={l}")
    # three train-mode calls moved the BatchNorm buffers of the WHOLE stack like three ordinary calls
    sd = d.state_dict()
    for k, v in o.D.items():
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == int(v) == 3, k
        elif k.endswith("running_mean") or k.endswith("running_var"):
            np.testing.assert_allclose(sd[k].cpu().numpy(), v.numpy(), rtol=1e-4, atol=2e-5, err_msg=k)
    for bad in (0, 4, 5, -1, 1.0, None):                 # no BatchNorm, the head, out of range, not an index
        with pytest.raises(ValueError):
            d.features(x.to(DEV), bad)
    for bad in (0, 4, 7):
        with pytest.raises(ValueError):
            build(S, feat_layer=bad, alpha_feat=1.0)
    with pytest.raises(ValueError):
        build(S, alpha_feat=1.0)                         # a weight without a layer


# ======================================================================================================================
# Off means off
# ======================================================================================================================
@pytest.mark.parametrize("graphed", [False, True])
def test_feature_off_is_bitwise_the_trainer_without_the_arguments(graphed):
    res = []
    for kw in ({}, dict(feat_layer=2, alpha_feat=0.0)):
        e, g, d, tr = build(64, **kw)
        fn = tr.train_step_graphed if graphed else tr.train_step
        n0 = ops.launch_count()
        losses = []
        for step in range(3):
            real, ez, er, ec = (t.to(DEV) for t in make_inputs(4, 64, 7064 + step))
            losses.append(fn(real, 60, ez, er, ec).cpu().clone())
        res.append((losses, full_state(e, g, d, tr), ops.launch_count() - n0, tr.loss_dict(epoch=60)))
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(a, b) and float(a[5]) == 0.0          # all 8 slots; slot 5 reads 0 with the feature off
    assert_same_state(res[0][1], res[1][1])
    assert res[0][2] == res[1][2], "the feature, switched off, changed the number of kernel launches"
    assert res[0][3] == res[1][3] and "feat_loss" not in res[1][3]


# ======================================================================================================================
# The iteration against ref_step
# ======================================================================================================================
_REF = {}


def ref_first_step(l):
    """(losses, D's state) of ref_step's first iteration at S = 64, B = 4, fp32, alpha_feat = 1: computed once per stage."""
    if l not in _REF:
        o = R.RefVAEGAN(img_size=64, seed=42)
        out = FR.ref_step(o, *make_inputs(4, 64, 7064), 60, feat_layer=l, alpha_feat=1.0)
        _REF[l] = (out, {k: v.detach().clone() for k, v in o.D.items()})
    return _REF[l]


@pytest.mark.parametrize("l", [1, 2, 3])
def test_first_step_with_the_feature_on_vs_ref_step(l):
    """Every loss within FIRST_STEP_TOL of tests/test_gpu_parity.py; feat_loss is evaluated after the two Discriminator
    updates, like g_loss_adv, and takes that entry's 5e-4."""
    ref, refD = ref_first_step(l)
    e, g, d, tr = build(64, feat_layer=l, alpha_feat=1.0)
    real, ez, er, ec = (t.to(DEV) for t in make_inputs(4, 64, 7064))
    got = tr.loss_dict(tr.train_step(real, 60, ez, er, ec), 60)
    tol = dict(FIRST_STEP_TOL, feat_loss=FIRST_STEP_TOL["g_loss_adv"])
    print({k: f"{got[k]:.6g} / {ref[k]:.6g} ({rel(got[k], ref[k]):.1e})" for k in tol})
    assert sorted(got) == sorted(tol)
    for k, t in tol.items():
        assert rel(got[k], ref[k]) <= t, f"l={l} {k}: hip {got[k]} ref_step {ref[k]}"
    sd = d.state_dict()
    for k, v in refD.items():
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == int(v) == 6, k          # 2 x (real, fake) + the feature pass on real + the pass on fake


@pytest.mark.parametrize("l", [2, 3])
def test_feature_gradient_path_in_isolation_vs_fp64_ref_step(l):
    """epoch = 0 (KL weight 0), alpha_adv = 0, alpha_pix = 0, alpha_feat = 1: every gradient that reaches the Encoder and the
    Generator went through the feature loss, the Discriminator's data-gradient chain below stage l and the instance-noise
    add.  Teacher-forced from the oracle's state; gradient = exp_avg / (1 - beta1) after the first Adam step.  Bound per
    tensor, as tests/test_gpu_parity.test_all_parameter_gradients_vs_fp64_oracle calibrates it: max error relative to the
    tensor's max <= max(1e-5, 4 x the CPU-fp32 ref_step's own error against the fp64 one) -- and, as there, with lr = 0 on
    both sides: the feature loss is evaluated AFTER the two Discriminator updates, and an Adam(t = 1) update is sign(g) lr
    per weight, so with lr > 0 any two fp32 implementations hold Discriminators that differ by +- 2 lr on the weights whose
    gradient is rounding noise (tests/test_gpu_parity.py, FIRST_STEP_TOL) and the gradient THROUGH that Discriminator
    inherits the difference: with lr = 2e-4 the Generator's main.10.weight measured 1.09e-5 against a bound of 1e-5 (CPU
    fp32: 2.3e-6) at l = 2.  The moments move with lr = 0 all the same.  l = 3: the gradient from above comes out of the
    head's backward; l = 2: out of a data-gradient GEMM.  Fails without the feature (no such argument)."""
    S, B = 64, 4
    kw = dict(alpha_adv=0.0, alpha_feat=1.0, alpha_pix=0.0, feat_layer=l)
    e, g, d, tr = build(S, lr=0.0, **kw)
    o = R.RefVAEGAN(img_size=S, seed=42, lr=0.0)
    sync_from_oracle(o, e, g, d, tr)
    o64 = oracle_twin_fp64(o)
    assert tr.opt_D.lr == 0.0 and o64.opt_D.lr == 0.0
    inp = make_inputs(B, S, 7064)
    FR.ref_step(o64, *inp, 0, **kw)
    FR.ref_step(o, *inp, 0, **kw)
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
            assert err_hip <= max(1e-5, 4 * err_cpu), f"l={l} {k}: hip err {err_hip:.2e}, cpu-fp32 err {err_cpu:.2e}"
    print(f"l={l}: worst gradient error / bound {worst:.3f}")


# ======================================================================================================================
# Graph replay and the capture key
# ======================================================================================================================
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_graphed_equals_eager_with_the_feature_on_and_recaptures_on_change(dtype):
    B, S = 4, 64
    (ee, ge, de, te), (eg, gg, dg, tg) = (build(S, dtype=dtype, feat_layer=2, alpha_feat=1.0) for _ in range(2))
    inputs = [[t.to(DEV) for t in make_inputs(B, S, 7064 + step)] for step in range(3)]

    def three_steps():
        out = []
        for real, ez, er, ec in inputs:
            le = te.train_step(real, 60, ez, er, ec).cpu().clone()
            lg = tg.train_step_graphed(real, 60, ez, er, ec).cpu().clone()
            assert torch.equal(le, lg), (le, lg)
            out.append(le)
        assert_same_state(full_state(ee, ge, de, te), full_state(eg, gg, dg, tg))
        return out

    first = three_steps()
    assert all(float(l[5]) > 0 for l in first)
    graph1 = tg._graph
    assert graph1 is not None and len(graph1[1]) == 1            # eager, capture + replay, replay: ONE graph
    # a new weight: the next call may not replay the old graph (the scalar is frozen in it)
    te.alpha_feat = tg.alpha_feat = 0.25
    second = three_steps()
    assert tg._graph is not graph1 and tg._graph.key != graph1.key
    graph2 = tg._graph
    # a new layer
    te.feat_layer = tg.feat_layer = 1
    third = three_steps()
    assert tg._graph is not graph2 and tg._graph.key != graph2.key
    assert float(third[0][5]) != float(second[0][5])             # the loss slot follows the new stage
    print([float(x[0][5]) for x in (first, second, third)])


def test_segmented_graph_with_a_reducer_equals_eager_with_the_feature_on():
    """The segmented (reducer) form: the iteration cut into hipGraph segments at the gradient hand-offs.  The feature adds no
    collective and no cut: the same 5 segments / 4 hand-offs as without it, and the same bits as the eager run."""
    res = []
    for graphed in (False, True):
        e, g, d, tr = build(64, feat_layer=3, alpha_feat=0.5, alpha_pix=0.5)
        tr.reducer = _LocalReducer()
        fn = tr.train_step_graphed if graphed else tr.train_step
        for step in range(3):
            real, ez, er, ec = (t.to(DEV) for t in make_inputs(4, 64, 7064 + step))
            l = fn(real, 60, ez, er, ec).cpu().clone()
        res.append((l, full_state(e, g, d, tr)))
        if graphed:
            assert len(tr._graph[1]) == 5 and len(tr._graph[2]) == 4
    assert torch.equal(res[0][0], res[1][0]) and float(res[0][0][5]) > 0
    assert_same_state(res[0][1], res[1][1])


# ======================================================================================================================
# bf16
# ======================================================================================================================
def test_bf16_first_step_feature_loss():
    """S = 64, B = 8, l = 2, bf16 engine.
    Route used: BOTH.  (a) against the f64 ref_step with the project's stated bf16 loss bound (3e-2: bf16 keeps 8
    significant bits; tests/test_gpu_parity.test_bf16_engine_tracks_fp32_oracle and tests/test_gpu_configs.py hold every
    first-iteration loss to it) -- the storage-rounding emulation (oracle/vaegan_ref_bf16.py) has no tap, so (b) the loss
    and the gradient-add are also re-derived in f64 from the engine's OWN stored bf16 activations and incoming gradient,
    read through engine.trace, with the kernel test's bounds."""
    S, B, l = 64, 8, 2
    e, g, d, tr = build(S, dtype="bf16", feat_layer=l, alpha_feat=1.0)
    inp = make_inputs(B, S, 7064)
    ref = FR.ref_step(R.RefVAEGAN(img_size=S, seed=42).double_(), *inp, 60, feat_layer=l, alpha_feat=1.0)
    d._engine.trace = []
    real, ez, er, ec = (t.to(DEV) for t in inp)
    got = tr.loss_dict(tr.train_step(real, 60, ez, er, ec), 60)
    trace, d._engine.trace = d._engine.trace, None
    print(f"bf16 feat_loss {got['feat_loss']:.6g}, f64 ref_step {ref['feat_loss']:.6g} (rel {rel(got['feat_loss'], ref['feat_loss']):.2e})")
    assert rel(got["feat_loss"], ref["feat_loss"]) <= 3e-2
    rec = [t for t in trace if t["what"] == "feat"]
    assert len(rec) == 1 and rec[0]["stage"] == l
    t = rec[0]
    assert t["f_fake"].dtype == t["f_real"].dtype == t["dA"].dtype == torch.bfloat16 and t["f_fake"].shape == (B, 8, 8, 256)
    a, b, d_in = t["f_fake"].double().cpu(), t["f_real"].double().cpu(), t["dA_in"].double().cpu()
    lref = FR.feat_mse(a, b)
    check(t["loss"], lref.view(1), 5 * U * lref, "bf16 in-step loss vs its own stored activations")
    assert float(t["loss"]) == got["feat_loss"]
    gref, dref = FR.feat_mse_grad_add(a, b, d_in, 1.0)
    check(t["dA"], dref, 3 * U * gref.abs() + U * dref.abs(), "bf16 in-step gradient-add", True)
