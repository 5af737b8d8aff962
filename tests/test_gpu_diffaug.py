"""GPU: the differentiable augmentation from the kernels up to the trainers: vg_diffaug_forward / _backward bit for bit against
the f32 restatement of the contract (tests/_diffaug_ref.py) on exactly representable inputs and within a counted bound of the
f64 restatement on random ones, the edges of shift and cutout and the parameter-safety promises on hand-made tables,
vg_diffaug_params against the header's formulas applied to ops.rand_u01's words, graph capture, and the three adversarial
trainers with the option off (bitwise the trainer without it), with the identity policy, against the oracle's iterations with
the transform applied (tests/_diffaug_ref.ref_step and its DCGAN / WGAN twins), graphed, checkpointed."""
import importlib
import os

import numpy as np
import pytest
import torch

import _diffaug_ref as DR
import siblings_ref as SR
import vaegan_ref as R
from _diffaug_ref import U, UB
from _inputs import make_inputs

import vaegan_amd as V
from test_gpu_featloss import assert_same_state, build, full_state
from test_gpu_parity import DEV, FIRST_STEP_TOL, oracle_twin_fp64, rel, sync_from_oracle
from test_gpu_siblings import build_gan, sib_inputs

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, os.cpu_count() or 1))

PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
G = importlib.import_module(PKG + ".geometry")
ops = importlib.import_module(PKG + ".ops")
TDT = {G.F32: torch.float32, G.BF16: torch.bfloat16}
F32, F64 = np.float32, np.float64
FWD_BWD = (("forward", ops.diffaug_forward, DR.forward), ("backward", ops.diffaug_backward, DR.backward))


def to_engine(x, dtype):
    """numpy [N, H, W, C] -> device [N, H, W, padc(C)] in the engine dtype, pad channels zero."""
    N, H, W, C = x.shape
    t = torch.zeros(N, H, W, G.padc(C, dtype), dtype=torch.float32)
    t[..., :C] = torch.from_numpy(np.asarray(x, dtype=F32))
    return t.to(TDT[dtype]).to(DEV)


def nan_like(x):
    return torch.full_like(x, float("nan"))


def stored(ref32, dtype):
    """The restatement's f32 result after the ONE rounding of the store."""
    return ref32 if dtype == G.F32 else DR.from_bf16(DR.to_bf16(ref32))


def run(fn, x, table, C, cut, dtype, **kw):
    """-> (real channels as f32 numpy, the whole output tensor); destination NaN-filled, pad channels checked zero."""
    out = nan_like(x)
    y = fn(x, torch.from_numpy(table).to(DEV), C, cut, dtype, out=out, **kw)
    assert y is out
    host = y.float().cpu().numpy()
    assert not host[..., C:].any() and not np.isnan(host[..., C:]).any(), "pad channels must be written as zero"
    return host[..., :C], y


# ======================================================================================================================
# Kernels, bit for bit on exact inputs
# ======================================================================================================================
EXACT_SHAPES = [(2, 2, 2, 3), (4, 8, 8, 3), (4, 16, 16, 4), (8, 64, 64, 3)]          # the last: four parts per image


@pytest.mark.parametrize("dtype", [G.F32, G.BF16])
@pytest.mark.parametrize("shape", EXACT_SHAPES)
def test_kernels_bitwise_vs_f32_restatement_on_exact_inputs(shape, dtype):
    """Inputs on which every intermediate is exact (tests/test_diffaug_cpu.py asserts it): the result does not depend on any
    order of summation or on contraction, so every bit is the contract's.  PB = N and PB = N / 2; with and without the
    whole-image sum where the table allows it."""
    N, H, W, C = shape
    assert ops.L.load().vg_diffaug_ws_floats(8, 64, 64) == 32
    for PB in (N, N // 2):
        x, t = DR.exact_case(N, H, W, C, PB, 100 + H + PB)
        cut = (DR.cut_size(H), DR.cut_size(W))
        X = to_engine(x, dtype)
        for name, fn, ref in FWD_BWD:
            got, _ = run(fn, X, t, C, cut, dtype)
            want = stored(ref(x, t, *cut, dt=F32), dtype)
            assert np.array_equal(got, want), f"{name} {shape} PB={PB}"
            got0, _ = run(fn, X, t, C, (0, 0), dtype)                                   # no cutout
            assert np.array_equal(got0, stored(ref(x, t, 0, 0, dt=F32), dtype)), f"{name} {shape} PB={PB} no cutout"
        t1 = t.copy()
        t1[:, 2] = 1.0                                                                   # k = 1: the sum's coefficient is 0
        for name, fn, ref in FWD_BWD:
            a, _ = run(fn, X, t1, C, cut, dtype, need_sum=False)
            b, _ = run(fn, X, t1, C, cut, dtype, need_sum=True)
            assert np.array_equal(a, b) and np.array_equal(a, stored(ref(x, t1, *cut, dt=F32, need_sum=False), dtype)), name


@pytest.mark.parametrize("shape", EXACT_SHAPES)
def test_adjoint_identity_on_exact_inputs(shape):
    """<T x, g> = <x, T' g> (beta = 0) with the dot products taken on the host in f64 from the f32 kernels' outputs: on these
    inputs both outputs are exact and so are the f64 products and sums, so the two sides are EQUAL."""
    N, H, W, C = shape
    x, t = DR.exact_case(N, H, W, C, N, 300 + H)
    g, _ = DR.exact_case(N, H, W, C, N, 400 + H)
    t[:, 0] = 0.0
    cut = (DR.cut_size(H), DR.cut_size(W))
    Tx, _ = run(ops.diffaug_forward, to_engine(x, G.F32), t, C, cut, G.F32)
    Tg, _ = run(ops.diffaug_backward, to_engine(g, G.F32), t, C, cut, G.F32)
    lhs = float((Tx.astype(F64) * g.astype(F64)).sum())
    rhs = float((x.astype(F64) * Tg.astype(F64)).sum())
    print(f"{shape}: <Tx, g> = {lhs}, <x, T'g> = {rhs}")
    assert lhs == rhs and (lhs != 0.0 or H < 8)          # (2 x 2: the draws may shift or cut everything away)


# ======================================================================================================================
# Hand-made tables: the edges
# ======================================================================================================================
def edge_table(H, W):
    rows = []

    def row(beta=0.0, s=1.0, k=1.0, ty=0.0, tx=0.0, cy=0.0, cx=0.0):
        rows.append([beta, s, k, ty, tx, cy, cx, 0.0])
    row()                                                            # 0: identity (cutout origin 0, 0 -- used with cut = 0 too)
    for ty, tx in ((1, 0), (-1, 0), (0, 1), (0, -1), (H - 1, -(W - 1)), (-(H - 1), W - 1)):
        row(ty=ty, tx=tx, cy=-100, cx=-100)                          # 1..6: shifts, cutout outside
    for ty, tx in ((H, 0), (0, -W), (1000, 1000), (-(2 ** 29), 2 ** 29)):
        row(ty=ty, tx=tx, cy=-100, cx=-100)                          # 7..10: everything shifted out
    row(cy=H, cx=0), row(cy=0, cx=W), row(cy=-100, cx=3)             # 11..13: cutout outside
    row(cy=-1, cx=-2), row(cy=H - 1, cx=W - 2), row(ty=1, tx=-1, cy=2, cx=2, s=0.5, k=2.0, beta=0.25)   # 14..16: clipped / inside
    for bad in (float("nan"), 1e30, -1e30, 2.0 ** 30):               # 17..24: NaN / huge entries
        row(ty=bad, tx=1, cy=-100, cx=-100)
        row(ty=1, tx=0, cy=bad, cx=0)
    row(tx=float("inf"), cy=0, cx=float("-inf"))                     # 25
    return np.array(rows, dtype=F32)


@pytest.mark.parametrize("dtype", [G.F32, G.BF16])
def test_edges_of_shift_and_cutout_and_bad_entries(dtype):
    H, W, C = 8, 8, 3
    t = edge_table(H, W)
    N = t.shape[0]
    x, _ = DR.exact_case(N, H, W, C, N, 77)
    X = to_engine(x, dtype)
    for cut in ((3, 4), (H, W), (0, 0)):
        for name, fn, ref in FWD_BWD:
            got, _ = run(fn, X, t, C, cut, dtype)
            want = stored(ref(x, t, *cut, dt=F32), dtype)
            bad = [n for n in range(N) if not np.array_equal(got[n], want[n])]
            assert not bad, f"{name} cut={cut}: rows {bad}"
            if cut == (3, 4):
                assert not got[7:11].any(), "a shift of the image's size or more leaves nothing"
                for n in (11, 12, 13):                               # a cutout outside the image removes nothing
                    assert np.array_equal(got[n], x[n])
                for n in (17, 19, 21, 23):                           # bad ty counts as 0: only tx = 1 acts
                    shifted = np.zeros_like(x[n])
                    if name == "forward":
                        shifted[:, :-1] = x[n][:, 1:]
                    else:
                        shifted[:, 1:] = x[n][:, :-1]
                    assert np.array_equal(got[n], shifted), n
                for n in (18, 20, 22, 24):                           # bad cy: no cutout for that image, ty = 1 acts
                    assert int((got[n] == 0).all(axis=-1).sum()) == W, n
            if cut == (H, W):
                assert not got[0].any() if name == "forward" else True    # origin 0, 0 and the full size: everything cut
    # the identity row without a cutout reproduces the input bit for bit, also on values that are not exact
    xr = np.random.default_rng(5).standard_normal((2, H, W, C)).astype(F32)
    Xr = to_engine(xr, dtype)
    for _, fn, _ in FWD_BWD:
        _, y = run(fn, Xr, DR.identity_table(2), C, (0, 0), dtype)
        assert torch.equal(y, Xr)


# ======================================================================================================================
# Random inputs and drawn tables against the f64 restatement
# ======================================================================================================================
RANDOM_SHAPES = [(2, 2, 2, 3), (4, 8, 8, 3), (3, 10, 6, 1), (4, 16, 16, 4), (8, 64, 64, 3), (2, 40, 40, 3), (2, 8, 8, 12)]


@pytest.mark.parametrize("dtype", [G.F32, G.BF16])
@pytest.mark.parametrize("shape", RANDOM_SHAPES)
def test_kernels_vs_f64_restatement_on_random_inputs(shape, dtype):
    """Bound, counted from the contract: an input reaches an output through at most K = _diffaug_ref.roundings(C, H, W) f32
    roundings (the whole-image sum's chain is the longest: C - 1 channel additions, 11 inside the part, one per part, then the
    quotient, 1 - k, the product, + beta and the two additions of out_c), each relative to a partial result that is at most
    A = |ks| |v| + (|k| + |ks|) mean_c |v| + |1 - k| mean |.| + |beta| (the terms of out_c before any cancellation, which also
    covers b = k - ks): |error| <= 1.01 K U A (1.01: the second-order terms of (1 + U)^K).  bf16 storage adds half a bf16 ulp
    of the result, UB (|ref| + bound), on top.  The inputs are representable in the storage type, the tables are DRAWN
    (ops.diffaug_params) so that the generator's ranges are what is exercised.  (2, 8, 8, 12): more than one 16-byte unit per
    pixel, the kernels' other path; (3, 10, 6, 1) with PB = N only (N is odd).  Measured: f32 at most 0.07 of the bound, bf16
    at most 0.995 (the half ulp of the store), and every element equal to the f32 restatement bit for bit."""
    N, H, W, C = shape
    rng = np.random.default_rng(sum(shape) + dtype)
    x = torch.from_numpy(rng.standard_normal(shape).astype(F32)).to(TDT[dtype]).float().numpy()
    X = to_engine(x, dtype)
    state = torch.tensor([1234 + H, 7], dtype=torch.int64, device=DEV)
    for PB in ((N, N // 2) if N % 2 == 0 else (N,)):
        t = ops.diffaug_params(state, PB, 31, H, W).cpu().numpy()
        cut = ops.diffaug_cut(31, H, W)
        K = DR.roundings(C, H, W)
        for name, fn, ref in FWD_BWD:
            got, _ = run(fn, X, t, C, cut, dtype)
            r64 = ref(x, t, *cut, dt=F64)
            bound = 1.01 * K * U * DR.abs_budget(x, t, *cut, bwd=(name == "backward"))
            if dtype == G.BF16:
                bound = bound + UB * (np.abs(r64) + bound)
            err = np.abs(got.astype(F64) - r64)
            ratio = float((err / np.maximum(bound, 1e-300)).max())
            same = float((got == stored(ref(x, t, *cut, dt=F32), dtype)).mean())
            print(f"{name} {shape} PB={PB}: max err {err.max():.3e}, max err/bound {ratio:.3f}, bitwise equal to the f32 "
                  f"restatement on {100 * same:.2f} % of the elements")
            assert np.isfinite(got).all() and (err <= bound).all(), f"{name}: max err/bound {ratio:.3f}"


# ======================================================================================================================
# The parameter generator
# ======================================================================================================================
def test_params_vs_header_formulas_on_rand_u01_words():
    B, H, W = 4096, 64, 48
    state = torch.tensor([99, 5], dtype=torch.int64, device=DEV)
    u = ops.rand_u01(8 * B, state, ops.DRAW_AUGMENT).cpu().numpy().astype(F64)
    u24 = np.round(u * 2.0 ** 24).astype(np.int64).reshape(B, 8)
    assert np.array_equal(u24.astype(F64) * 2.0 ** -24, u.reshape(B, 8))
    for policy in (31, 0, 7, 8, 16, 30, 29, 27, 23, 15):
        got = ops.diffaug_params(state, B, policy, H, W, out=torch.full((B, 8), float("nan"), device=DEV)).cpu().numpy()
        assert np.array_equal(got, DR.params_from_u24(u24, policy, H, W)), policy
    p = ops.diffaug_params(state, B, 31, H, W).cpu().numpy()
    assert -0.5 <= p[:, 0].min() and p[:, 0].max() < 0.5 and 0 <= p[:, 1].min() and p[:, 1].max() < 2
    assert 0.5 <= p[:, 2].min() and p[:, 2].max() <= 1.5 and not p[:, 7].any()
    for col, lo, hi in ((3, -8, 8), (4, -6, 6), (5, -16, 48), (6, -12, 36)):          # both ends of each integer range are hit
        assert p[:, col].min() == lo and p[:, col].max() == hi, col
        assert np.array_equal(p[:, col], np.round(p[:, col]))
    # another iteration, another table; the same state, the same table
    state2 = torch.tensor([99, 6], dtype=torch.int64, device=DEV)
    assert not np.array_equal(ops.diffaug_params(state2, B, 31, H, W).cpu().numpy(), p)
    assert np.array_equal(ops.diffaug_params(state.clone(), B, 31, H, W).cpu().numpy(), p)


@pytest.mark.parametrize("dtype", [G.F32, G.BF16])
def test_params_and_apply_are_capturable_and_draw_a_new_table_each_replay(dtype):
    N, H, W, C = 8, 64, 64, 3
    aug = V.DiffAugment()
    x = np.random.default_rng(1).standard_normal((N, H, W, C)).astype(F32)
    X = to_engine(x, dtype)
    noise = ops.NoiseStream(DEV, 4242)
    table, y, dx = torch.zeros(N // 2, 8, device=DEV), nan_like(X), nan_like(X)
    aug.forward(X, aug.draw(noise.state, N // 2, H, W), C, dtype)                       # sizes the workspace
    noise.set_state(torch.tensor([4242, 0]))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            noise.advance()
            aug.draw(noise.state, N // 2, H, W, out=table)
            aug.forward(X, table, C, dtype, out=y)
            aug.backward(y, table, C, dtype, out=dx)
    torch.cuda.current_stream().wait_stream(s)
    seen = []
    for it in range(1, 4):
        g.replay()
        torch.cuda.synchronize()
        assert int(noise.state[1]) == it
        eager = ops.NoiseStream(DEV, 4242)
        eager.set_state(torch.tensor([4242, it]))
        te = aug.draw(eager.state, N // 2, H, W)
        ye = aug.forward(X, te, C, dtype)
        assert torch.equal(te, table) and torch.equal(ye, y) and torch.equal(aug.backward(ye, te, C, dtype), dx)
        seen.append(table.cpu().clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


# ======================================================================================================================
# VAEGANTrainer
# ======================================================================================================================
S, B = 64, 4
TOL3 = {k: 3 * v for k, v in FIRST_STEP_TOL.items()}          # the feature-loss tests' bounds times 3, the largest |k s|


def step_inputs(step=0):
    return [t.to(DEV) for t in make_inputs(B, S, 7064 + step)]


@pytest.mark.parametrize("graphed", [False, True])
def test_augment_none_is_bitwise_the_trainer_without_the_argument(graphed):
    res = []
    for kw in ({}, dict(augment=None)):
        e, g, d, tr = build(S, **kw)
        fn = tr.train_step_graphed if graphed else tr.train_step
        n0 = ops.launch_count()
        losses = [fn(*step_inputs(step)[:1], 60, *step_inputs(step)[1:]).cpu().clone() for step in range(3)]
        res.append((losses, full_state(e, g, d, tr), ops.launch_count() - n0))
        assert tr.aug_params is None and tr.noise is None            # nothing allocated
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(a, b)
    assert_same_state(res[0][1], res[1][1])
    assert res[0][2] == res[1][2], "augment=None changed the number of kernel launches"


def test_identity_policy_gives_the_unaugmented_step_bitwise():
    res = []
    for kw in ({}, dict(augment="")):
        e, g, d, tr = build(S, **kw)
        losses = []
        n0 = ops.launch_count()
        for step in range(2):
            real, ez, er, ec = step_inputs(step)
            losses.append(tr.train_step(real, 60, ez, er, ec).cpu().clone())
        res.append((losses, full_state(e, g, d, tr), ops.launch_count() - n0))
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(a, b)
    assert_same_state(res[0][1], res[1][1])
    # per iteration: the table, the forward apply, the backward apply (no reduce launches: no contrast bit)
    assert res[1][2] - res[0][2] == 2 * 3
    assert torch.equal(tr.aug_params.cpu(), torch.from_numpy(DR.identity_table(B)))


def test_construction_checks():
    with pytest.raises(ValueError):
        build(S, augment="colour")
    e, g, d, tr = build(S, augment=V.DiffAugment("color"))
    assert tr.augment.bits == 7
    with pytest.raises(ValueError):
        importlib.import_module(PKG + ".augment").check_dtype(G.FP8)


@pytest.mark.parametrize("policy", ["color,translation,cutout", "translation"])
def test_first_step_with_augmentation_vs_ref_step(policy):
    """fp32, S = 64, B = 4: every first-step loss against tests/_diffaug_ref.ref_step (the oracle's iteration with the
    transform applied in torch) fed the table the trainer drew, within 3 x FIRST_STEP_TOL.
    Measured on an MI355X (relative difference hip / ref_step): full policy: recon 0, kl 2.3e-7, d_loss_1 2.4e-7, d_loss_2
    4.3e-7, g_loss_adv 1.9e-7, total 2.2e-7; translation only: d_loss_1 2.3e-7, d_loss_2 3.1e-5, g_loss_adv 3.2e-4 (bound
    1.5e-3), total 7.7e-5 -- the two losses evaluated after Adam updates of D carry the sign(g) lr noise FIRST_STEP_TOL allows
    for."""
    e, g, d, tr = build(S, augment=policy)
    real, ez, er, ec = step_inputs()
    got = tr.loss_dict(tr.train_step(real, 60, ez, er, ec), 60)
    table = tr.aug_params.cpu().numpy()
    assert np.array_equal(table[:, 3:7], np.round(table[:, 3:7])) and tr.noise is not None and int(tr.noise.state[1]) == 1
    if "color" in policy:
        assert (table[:, :3] != DR.identity_table(B)[:, :3]).all()
    ref = DR.ref_step(R.RefVAEGAN(img_size=S, seed=42), *make_inputs(B, S, 7064), 60, table, DR.cut_of(tr.augment.bits, S, S))
    plain = R.RefVAEGAN(img_size=S, seed=42).train_step(*make_inputs(B, S, 7064), 60)
    print({k: f"{got[k]:.6g} / {ref[k]:.6g} ({rel(got[k], ref[k]):.1e})" for k in TOL3})
    for k, t in TOL3.items():
        assert rel(got[k], ref[k]) <= t, f"{k}: hip {got[k]} ref_step {ref[k]}"
    print(f"d_loss_1 without augmentation: {plain['d_loss_1']:.6g}")
    assert ref["d_loss_1"] != plain["d_loss_1"], "the table must matter for the check to mean anything"


def test_gradient_path_through_the_adjoint_in_isolation_vs_fp64_ref_step():
    """epoch = 0 (KL weight 0), alpha_pix = 0, alpha_adv = 1: every gradient that reaches the Generator and the Encoder went
    through the Discriminator's input gradient, vg_diffaug_backward and the instance-noise add.  Teacher-forced, lr = 0, bound
    per tensor as tests/test_gpu_featloss.test_feature_gradient_path_in_isolation_vs_fp64_ref_step calibrates it, times 3:
    max error relative to the tensor's max <= 3 max(1e-5, 4 x the CPU-fp32 ref_step's own error against the fp64 one).  A
    wrong adjoint (a shift in the wrong direction, a mask at the wrong end) is an O(1) error here.  Measured: worst tensor at
    0.10 of its bound."""
    kw = dict(alpha_adv=1.0, alpha_pix=0.0)
    e, g, d, tr = build(S, lr=0.0, augment="color,translation,cutout", **kw)
    o = R.RefVAEGAN(img_size=S, seed=42, lr=0.0)
    sync_from_oracle(o, e, g, d, tr)
    o64 = oracle_twin_fp64(o)
    inp = make_inputs(B, S, 7064)
    tr.train_step(*(t.to(DEV) for t in inp[:1]), 0, *(t.to(DEV) for t in inp[1:]))
    table, cut = tr.aug_params.cpu().numpy(), DR.cut_of(31, S, S)
    DR.ref_step(o64, *inp, 0, table, cut, **kw)
    DR.ref_step(o, *inp, 0, table, cut, **kw)
    worst = 0.0
    for m, opt, st, st64 in ((e, tr.opt_E, o.E, o64.E), (g, tr.opt_G, o.G, o64.G)):
        hsd = opt.state_dict()["state"]
        keys = R.trainable_keys(st)
        for i, k in enumerate(keys):
            if k.endswith("conv.bias") and m is e:
                continue                    # exactly-zero true gradient in front of BatchNorm: rounding noise everywhere
            r64, r32 = st64[k].grad.double(), st[k].grad.double()
            hip = hsd[i]["exp_avg"].double().cpu().reshape(r64.shape) / (1 - opt.betas[0])
            scale = float(r64.abs().max())
            assert scale > 0, k
            err_hip, err_cpu = float((hip - r64).abs().max()) / scale, float((r32 - r64).abs().max()) / scale
            worst = max(worst, err_hip / (3 * max(1e-5, 4 * err_cpu)))
            assert err_hip <= 3 * max(1e-5, 4 * err_cpu), f"{k}: hip err {err_hip:.2e}, cpu-fp32 err {err_cpu:.2e}"
    print(f"worst gradient error / bound {worst:.3f}")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_graphed_equals_eager_with_augmentation_and_recaptures_on_a_policy_change(dtype):
    (ee, ge, de, te), (eg, gg, dg, tg) = (build(S, dtype=dtype, augment="color,translation,cutout") for _ in range(2))
    inputs = [step_inputs(step) for step in range(3)]

    def three_steps():
        tables = []
        for real, ez, er, ec in inputs:
            le = te.train_step(real, 60, ez, er, ec).cpu().clone()
            lg = tg.train_step_graphed(real, 60, ez, er, ec).cpu().clone()
            assert torch.equal(le, lg), (le, lg)
            assert torch.equal(te.aug_params, tg.aug_params)
            tables.append(tg.aug_params.cpu().clone())
        assert_same_state(full_state(ee, ge, de, te), full_state(eg, gg, dg, tg))
        assert not torch.equal(tables[1], tables[2])                 # a replay draws a new table
        return tables

    three_steps()
    graph1 = tg._graph
    assert graph1 is not None and len(graph1[1]) == 1               # eager, capture + replay, replay: ONE graph
    te.augment = tg.augment = V.DiffAugment("color")
    tables = three_steps()
    assert tg._graph is not graph1 and tg._graph.key != graph1.key
    assert not tables[0][:, 3:7].any()                               # no translation, no cutout any more
    # device-drawn noise and augmentation share the stream
    for _ in range(3):
        real = inputs[0][0]
        assert torch.equal(te.train_step(real, 60).cpu(), tg.train_step_graphed(real, 60).cpu())
    assert_same_state(full_state(ee, ge, de, te), full_state(eg, gg, dg, tg))


def test_feature_loss_and_paired_step_with_augmentation_vs_ref_step():
    """The feature loss compares D_l of the real image and of its reconstruction: both carry the SAME row of the table.  The
    paired step feeds the Encoder another image.  Losses within 3 x FIRST_STEP_TOL (feat_loss: g_loss_adv's entry, as in
    tests/test_gpu_featloss.py).  Measured: g_loss_adv 3.9e-5, feat_loss 9.7e-6, total 4.2e-6, the others <= 3e-7."""
    kw = dict(feat_layer=2, alpha_feat=1.0)
    e, g, d, tr = build(S, augment="color,translation,cutout", **kw)
    real, ez, er, ec = make_inputs(B, S, 7064)
    noisy = (real + 0.3 * torch.randn(real.shape, generator=torch.Generator().manual_seed(3))).clamp(-1, 1)
    got = tr.loss_dict(tr.train_step(real.to(DEV), 60, ez.to(DEV), er.to(DEV), ec.to(DEV), noisy=noisy.to(DEV)), 60)
    ref = DR.ref_step(R.RefVAEGAN(img_size=S, seed=42), real, ez, er, ec, 60, tr.aug_params.cpu().numpy(), DR.cut_of(31, S, S),
                      noisy=noisy, **kw)
    tol = dict(TOL3, feat_loss=TOL3["g_loss_adv"])
    print({k: f"{got[k]:.6g} / {ref[k]:.6g} ({rel(got[k], ref[k]):.1e})" for k in tol})
    for k, t in tol.items():
        assert rel(got[k], ref[k]) <= t, f"{k}: hip {got[k]} ref_step {ref[k]}"


def test_checkpoint_round_trip_continues_bitwise(tmp_path):
    e, g, d, tr = build(S, augment="color,translation,cutout")
    for step in range(2):
        tr.train_step(*step_inputs(step)[:1], 60, *step_inputs(step)[1:])
    path = os.path.join(tmp_path, "ck.pt")
    tr.save_checkpoint(path)
    sd = torch.load(path, weights_only=True)
    assert "augment" not in sd and int(sd["noise"][1]) == 2         # nothing new in the payload: the noise state has it all
    want = tr.train_step(*step_inputs(2)[:1], 60, *step_inputs(2)[1:]).cpu().clone()
    want_table, want_state = tr.aug_params.cpu().clone(), full_state(e, g, d, tr)
    V.configure_seed(4321)                                          # the resuming process has another torch seed
    e2 = V.Encoder([3, S, S], 100)
    g2, d2 = V.Generator(nz=100, img_size=S), V.Discriminator(img_size=S)
    e2.to(DEV), g2.to(DEV), d2.to(DEV)
    tr2 = V.VAEGANTrainer(e2, g2, d2, *(V.Adam(m.parameters(), lr=2e-4) for m in (e2, g2, d2)), augment="color,translation,cutout")
    tr2.train()
    tr2.load_checkpoint(path)
    got = tr2.train_step(*step_inputs(2)[:1], 60, *step_inputs(2)[1:]).cpu().clone()
    assert torch.equal(tr2.aug_params.cpu(), want_table) and torch.equal(got, want)
    assert_same_state(full_state(e2, g2, d2, tr2), want_state)


# ======================================================================================================================
# DCGANTrainer / WGANTrainer
# ======================================================================================================================
def gan_state(g, d, tr):
    torch.cuda.synchronize()
    out = {f"{n}.{k}": v.cpu().clone() for n, m in (("G", g), ("D", d)) for k, v in m.state_dict().items()}
    for n, o in (("G", tr.opt_G), ("D", tr.opt_D)):
        for a in ("flat_p", "exp_avg", "exp_avg_sq"):
            out[f"opt_{n}.{a}"] = getattr(o, a).cpu().clone()
    return out


def gan_args(which, step):
    real, _, _, noises = sib_inputs(B, S, step)
    if which == "dcgan":
        return (real.to(DEV), noises[0].to(DEV))
    return (real.to(DEV), torch.stack(noises[:5]).to(DEV), noises[5].to(DEV))


CLS = {"dcgan": V.DCGANTrainer, "wgan": V.WGANTrainer}


@pytest.mark.parametrize("which", ["dcgan", "wgan"])
def test_sibling_augment_none_and_identity_policy_are_bitwise_the_plain_trainer(which):
    res = []
    for kw in ({}, dict(augment=None), dict(augment="")):
        g, d, tr = build_gan(S, CLS[which], **kw)
        n0 = ops.launch_count()
        losses = [tr.train_step(*gan_args(which, step)).cpu().clone() for step in range(2)]
        res.append((losses, gan_state(g, d, tr), ops.launch_count() - n0))
        if not kw or kw["augment"] is None:
            assert tr.aug_params is None and tr.aug_noise is None
    for other in res[1:]:
        for a, b in zip(res[0][0], other[0]):
            assert torch.equal(a, b)
        assert_same_state(res[0][1], other[1])
    assert res[0][2] == res[1][2] and res[2][2] > res[0][2]


def test_dcgan_first_step_with_augmentation_vs_siblings_ref():
    """errD_real, errD_fake, errG within 3 x the first-step bounds of tests/test_gpu_siblings.check_dcgan.  Measured: 8.6e-7,
    1.2e-6, 3.7e-7."""
    g, d, tr = build_gan(S, V.DCGANTrainer, augment="color,translation,cutout")
    real, _, _, noises = sib_inputs(B, S, 0)
    got = tr.train_step(real.to(DEV), noises[0].to(DEV))[:3].tolist()
    ref = DR.ref_dcgan_step(SR.RefDCGAN(img_size=S, seed=42), real, noises[0], tr.aug_params.cpu().numpy(), DR.cut_of(31, S, S))
    plain = SR.RefDCGAN(img_size=S, seed=42).train_step(real, noises[0])
    for i, (n, tol) in enumerate((("errD_real", 1e-4), ("errD_fake", 1e-4), ("errG", 5e-4))):
        print(f"{n}: hip {got[i]:.6g} ref {ref[n]:.6g} ({rel(got[i], ref[n]):.1e}); without augmentation {plain[n]:.6g}")
        assert rel(got[i], ref[n]) <= 3 * tol, n
    assert ref["errD_real"] != plain["errD_real"]


def test_wgan_first_step_with_augmentation_vs_siblings_ref():
    """d_loss, g_loss within 3 x the absolute first-step bound of tests/test_gpu_siblings.check_wgan (5e-5).  Measured: 3.3e-7
    both."""
    g, d, tr = build_gan(S, V.WGANTrainer, augment="color,translation,cutout")
    real, _, _, noises = sib_inputs(B, S, 0)
    got = tr.train_step(real.to(DEV), torch.stack(noises[:5]).to(DEV), noises[5].to(DEV))[:2].tolist()
    ref = DR.ref_wgan_step(SR.RefWGAN(img_size=S, seed=42), real, noises[:5], noises[5], tr.aug_params.cpu().numpy(),
                           DR.cut_of(31, S, S))
    for i, n in enumerate(("d_loss", "g_loss")):
        print(f"{n}: hip {got[i]:.6g} ref {ref[n]:.6g} (abs {abs(got[i] - ref[n]):.1e})")
        assert abs(got[i] - ref[n]) <= 3 * 5e-5, n


@pytest.mark.parametrize("which", ["dcgan", "wgan"])
def test_sibling_graph_replay_with_augmentation_equals_eager_and_state_round_trips(which):
    res = []
    for graphed in (False, True):
        g, d, tr = build_gan(S, CLS[which], augment="color,translation,cutout")
        fn = tr.step_graphed if graphed else tr.train_step
        outs, tables = [], []
        for step in range(4):
            outs.append(fn(*gan_args(which, step)).clone())
            tables.append(tr.aug_params.clone())
        res.append((torch.stack(outs).cpu(), torch.stack(tables).cpu(), gan_state(g, d, tr), tr))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert not torch.equal(res[0][1][2], res[0][1][3])               # a new table per step, also under replay
    assert_same_state(res[0][2], res[1][2])
    # the stream's state saved and restored: the next table is the one the original would have drawn
    tr = res[0][3]
    st = tr.augment_state()
    assert int(st[1]) == 4
    tr.train_step(*gan_args(which, 4))
    want = tr.aug_params.cpu().clone()
    V.configure_seed(777)
    g2, d2, tr2 = build_gan(S, CLS[which], augment="color,translation,cutout")
    tr2.load_augment_state(st)
    tr2.train_step(*gan_args(which, 4))
    assert torch.equal(tr2.aug_params.cpu(), want)
