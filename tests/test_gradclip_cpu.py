"""No GPU: the restatement the gradient-clipping kernels are tested against (tests/_gradclip_ref.py) is itself checked --
against torch.nn.utils.clip_grad_norm_ in f64, at its non-finite edge cases, through the oracle's iteration -- and the exported
symbols, the constants, the host-side argument checks of vg_grad_norm_clip / vg_adam_apply_clip and the validation of
max_grad_norm against the built library and package."""
import ctypes
import math
import os
import re
from importlib import import_module

import numpy as np
import pytest
import torch

import _gradclip_ref as GR
import vaegan_ref as R
from _inputs import make_inputs
from vaegan_amd import clip_grad_norm_  # noqa: F401  (this file is about the feature: without it nothing here is collected)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
F32 = np.float32
INF = math.inf


# ---- the restatement against torch ------------------------------------------------------------------------------------
SIZE_MIXES = [[1], [3], [1, 3], [7, 1, 64], [3, 1000, 1, 17], [4096], [5, 5, 5, 5, 5]]


def test_f64_restatement_equals_torch_clip_grad_norm():
    """norm, coefficient and the scaled gradients against torch's function on f64 CPU tensors (grad_scale = 1).  torch takes
    the norm of the per-tensor norms, the restatement one sum of squares: a handful of f64 roundings apart (worst seen 6.4e-15
    over 50 random cases), held to rtol 1e-12."""
    rng = np.random.default_rng(5)
    worst = 0.0
    for case in range(56):
        sizes = SIZE_MIXES[case % len(SIZE_MIXES)]
        gs = [GR.float_grads(n, 1000 + 10 * case + i) for i, n in enumerate(sizes)]       # f32 values: the squares are exact
        flat = np.concatenate(gs)
        norm0, _ = GR.norm_coef_f64(flat, 1.0, INF)
        max_norm = float(norm0 * (rng.uniform(0.05, 0.95) if case % 2 else rng.uniform(1.05, 20.0)))   # both sides of the norm
        params = [torch.nn.Parameter(torch.zeros(n, dtype=torch.float64)) for n in sizes]
        for p, g in zip(params, gs):
            p.grad = torch.from_numpy(g.astype(np.float64))
        t_norm = float(torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2, error_if_nonfinite=False))
        norm, c = GR.norm_coef_f64(flat, 1.0, max_norm)
        assert (c < 1.0) == (case % 2 == 1)
        worst = max(worst, abs(norm - t_norm) / t_norm)
        np.testing.assert_allclose(norm, t_norm, rtol=1e-12, atol=0)
        got = np.concatenate([p.grad.numpy() for p in params])
        np.testing.assert_allclose(flat.astype(np.float64) * c, got, rtol=1e-12, atol=0)
        if c == 1.0:
            assert np.array_equal(got, flat.astype(np.float64))
    print(f"f64 restatement against torch.nn.utils.clip_grad_norm_: worst relative difference of the norm {worst:.3e}")


def _torch_f32(g, max_norm):
    p = torch.nn.Parameter(torch.zeros(g.size))
    p.grad = torch.from_numpy(g.copy())
    with np.errstate(all="ignore"):
        norm = torch.nn.utils.clip_grad_norm_([p], max_norm, norm_type=2, error_if_nonfinite=False)
    return float(norm), p.grad.numpy()


def test_non_finite_and_zero_cases_equal_torch_exactly():
    base = np.array([1.0, -2.0, 2.0, 0.0, 4.0], dtype=F32)          # norm 5: exact in every format
    # a NaN element: norm NaN, coefficient NaN, every gradient NaN
    g = base.copy()
    g[1] = np.nan
    norm, coef = GR.norm_coef(g, 1.0, 1.0)
    t_norm, t_g = _torch_f32(g, 1.0)
    assert np.isnan(norm) and np.isnan(coef) and np.isnan(t_norm) and np.isnan(t_g).all()
    assert np.isnan(g * coef).all()
    assert np.isnan(GR.norm_coef(g, 1.0, INF)[1])
    # an infinite element: norm inf, coefficient 0 -> the infinite element NaN, the others (signed) 0
    g = base.copy()
    g[2] = np.inf
    norm, coef = GR.norm_coef(g, 1.0, 1.0)
    t_norm, t_g = _torch_f32(g, 1.0)
    assert norm == np.inf == t_norm and coef == 0.0 and GR.bits(coef)[0] == 0
    with np.errstate(invalid="ignore"):
        mine = g * coef
    assert GR.same_bits(mine, t_g) and np.isnan(mine[2]) and (np.delete(mine, 2) == 0).all()
    # ... and with max_norm = inf: inf / inf, NaN, as torch
    t_norm, t_g = _torch_f32(g, INF)
    assert np.isnan(GR.norm_coef(g, 1.0, INF)[1]) and np.isnan(t_g).all()
    # squares that overflow f32 but not f64: torch's f32 norm is inf, this one finite -- the one place the two differ in
    # kind, by the wider reduction the contract states
    g = np.array([3e30, 4e30], dtype=F32)
    norm, coef = GR.norm_coef(g, 1.0, 1.0)
    assert np.isfinite(norm) and abs(float(norm) / 5e30 - 1.0) < 1e-6 and 0.0 < coef < 1e-30
    # the all-zero gradient: norm 0, coefficient 1 (1 / 1e-6 clamped), gradients unchanged
    g = np.zeros(7, dtype=F32)
    norm, coef = GR.norm_coef(g, 1.0, 1.0)
    t_norm, t_g = _torch_f32(g, 1.0)
    assert norm == 0.0 == t_norm and coef == 1.0 and GR.same_bits(g * coef, t_g)
    # max_norm = 0: coefficient 0 also for the zero gradient (0 / 1e-6)
    assert GR.norm_coef(g, 1.0, 0.0)[1] == 0.0 and GR.norm_coef(base, 1.0, 0.0)[1] == 0.0
    assert _torch_f32(base, 0.0)[1].tolist() == [0.0, -0.0, 0.0, 0.0, 0.0]
    # max_norm = inf, finite norm: coefficient exactly 1
    assert GR.norm_coef(base, 1.0, INF) == (F32(5.0), F32(1.0))
    assert GR.norm_coef(base, 0.5, INF) == (F32(2.5), F32(1.0)) and GR.norm_coef(base, -0.5, 1.0)[0] == F32(2.5)


def test_integer_inputs_meet_the_exactness_premise_and_f32_torch_agrees_on_small_ones():
    for n, seed in ((1, 1), (5, 2), (1029, 3), (512 * 256 * 16 + 3 * 1024 + 1, 4)):
        g = GR.int_grads(n, seed)
        GR.check_conditions(g)
        assert set(np.unique(g)) <= set(float(v) for v in range(-3, 4))
        S = GR.sum_squares(g)
        assert S == float(int(S)) == float(np.sum(g[::-1].astype(np.float64) ** 2))          # any order, the same integer
    g = GR.int_grads(1029, 3)
    norm, coef = GR.norm_coef(g, 1.0, 10.0)
    t_norm, t_g = _torch_f32(g, 10.0)
    assert GR.ulp_distance(norm, t_norm) <= 1 and coef < 1.0
    np.testing.assert_allclose(g * coef, t_g, rtol=4 * 2.0 ** -24, atol=0)       # torch's f32 coefficient, then one product
    with pytest.raises(AssertionError):
        GR.check_conditions(GR.float_grads(16, 1))


def test_coefficient_one_returns_the_unclipped_steps_bits():
    g = torch.Generator().manual_seed(3)
    p0, grads = torch.randn(1029, generator=g), [torch.randn(1029, generator=g) for _ in range(3)]
    for scale in (1.0, 1.0 / 3.0):
        assert GR.clip_scale(scale, 1.0) == F32(scale) == GR.clip_scale(scale, None)
        plain = GR.clipped_adam_step(p0, grads, 2e-4, (0.9, 0.999), 1e-8, scale, None)
        ones = GR.clipped_adam_step(p0, grads, 2e-4, (0.9, 0.999), 1e-8, scale, [1.0] * 3)
        clipped = GR.clipped_adam_step(p0, grads, 2e-4, (0.9, 0.999), 1e-8, scale, [0.25, 0.5, 0.75])
        for a, b, c in zip(plain, ones, clipped):
            assert torch.equal(a, b) and not torch.equal(a, c)
    # with grad_scale = 1 the gradient handed to Adam is torch's g.mul_(coef)
    coef = F32(0.3)
    assert GR.clip_scale(1.0, coef) == coef
    a = GR.clipped_adam_step(p0, grads[:1], 2e-4, (0.9, 0.999), 1e-8, 1.0, [coef])
    q = torch.nn.Parameter(p0.clone())
    q.grad = grads[0].clone().mul_(torch.tensor(coef))
    opt = torch.optim.Adam([q], lr=2e-4, foreach=False)
    opt.step()
    assert torch.equal(a[0], q.detach())


# ---- the oracle's iteration with torch's clipping ---------------------------------------------------------------------
S, B = 64, 2


def _state(m):
    return [t.detach().clone() for st in (m.E, m.G, m.D) for t in st.values()] + \
        [t.clone() for o in (m.opt_E, m.opt_G, m.opt_D) for t in o.exp_avg + o.exp_avg_sq]


def test_ref_step_with_an_infinite_max_norm_is_the_oracles_own_step_and_a_small_one_clips():
    real, ez, er, ec = make_inputs(B, S, 7000)
    own = R.RefVAEGAN(img_size=S)
    want = own.train_step(real, ez, er, ec, 60)
    mon = R.RefVAEGAN(img_size=S)
    got = GR.ref_step(mon, real, ez, er, ec, 60, max_norm=INF)
    for k, v in want.items():
        assert got[k] == v, k
    for a, b in zip(_state(own), _state(mon)):
        assert torch.equal(a, b)
    off = R.RefVAEGAN(img_size=S)
    GR.ref_step(off, real, ez, er, ec, 60, max_norm=None)
    for a, b in zip(_state(own), _state(off)):
        assert torch.equal(a, b)
    # a small max norm: the coefficients are below 1 and the parameters move differently
    clipped = R.RefVAEGAN(img_size=S)
    got = GR.ref_step(clipped, real, ez, er, ec, 60, max_norm=1e-3)
    for k in GR.NETS:
        norm, coef = GR.norm_coef(got["seen"][k].numpy(), 1.0, 1e-3)
        print(f"f32 oracle, network {k}: torch's f32 norm {got[f'grad_norm_{k}']:.9g}, f64 sum of the same gradient {norm:.9g}")
        assert coef < 1.0 and got[f"grad_norm_{k}"] > 1.0
    assert got["recon_loss"] == want["recon_loss"] and got["d_loss_1"] == want["d_loss_1"]      # forward of the first pass
    assert got["d_loss_2"] != want["d_loss_2"]                                                   # after a clipped D update
    changed = [not torch.equal(a, b) for a, b in zip(_state(own), _state(clipped))]
    assert any(changed)
    for st_own, st_clip in ((own.E, clipped.E), (own.G, clipped.G), (own.D, clipped.D)):
        k = R.trainable_keys(st_own)[0]
        assert not torch.equal(st_own[k], st_clip[k]), k
    # dict form: only the named network's step changes
    only_d = R.RefVAEGAN(img_size=S)
    got_d = GR.ref_step(only_d, real, ez, er, ec, 60, max_norm={"D": 1e-3})
    assert "grad_norm_D" in got_d and "grad_norm_E" not in got_d and "grad_norm_G" not in got_d
    k = R.trainable_keys(own.D)[0]
    assert torch.equal(only_d.D[k], clipped.D[k]) and not torch.equal(only_d.D[k], own.D[k])


def test_f64_ref_step_reports_norm_coef_of_the_gradients_it_saw():
    """The f64 oracle: torch's norm of per-tensor norms against the restatement's one sum over the same f64 gradients, the
    rtol 1e-12 of the first test.  (torch's f32 CPU reduction over these 10^6 .. 10^7 elements is itself 1e-4 off the f64
    value, printed above -- which is why the kernel reduces in f64 and why the f32 oracle is no yardstick for the norm.)"""
    real, ez, er, ec = make_inputs(B, S, 7000)
    for max_norm, d_iters in ((1e-3, 2), ({"E": 5.0, "D": INF}, 1)):
        m = R.RefVAEGAN(img_size=S).double_()
        got = GR.ref_step(m, real, ez, er, ec, 60, max_norm=max_norm, d_iters=d_iters)
        nets = GR.NETS if not isinstance(max_norm, dict) else tuple(max_norm)
        assert sorted(k for k in got if k.startswith("grad_norm_")) == sorted(f"grad_norm_{k}" for k in nets)
        for k in nets:
            assert got["seen"][k].dtype == torch.float64
            norm, _ = GR.norm_coef_f64(got["seen"][k].numpy(), 1.0, INF)
            np.testing.assert_allclose(got[f"grad_norm_{k}"], norm, rtol=1e-12, atol=0)


# ---- C ABI on the host ------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_the_abi_version_moved():
    L = import_module(PKG + "._lib")
    lib = L.load()
    src = open(os.path.join(ROOT, "include", "vaegan_hip.h")).read()
    assert int(re.search(r"#define\s+VG_ABI_VERSION\s+(\d+)", src).group(1)) == L.ABI_VERSION >= 24
    assert lib.vg_abi_version() == L.ABI_VERSION
    for name in ("vg_grad_norm_clip", "vg_adam_apply_clip"):
        assert name in L.SIGNATURES and name in src and getattr(lib, name) is not None
    assert "Gradient-norm clipping" in src
    assert int(re.search(r"#define\s+VG_GNORM_MAX\s+(\d+)", src).group(1)) == L.VG_GNORM_MAX
    assert int(re.search(r"#define\s+VG_GNORM_PARTS\s+(\d+)", src).group(1)) == L.VG_GNORM_PARTS
    assert L.VG_GNORM_MAX >= 3                                       # the three optimizers of the VAE-GAN in one call
    V = import_module("vaegan_amd")
    O = import_module(PKG + ".optim")
    assert "clip_grad_norm_" in V.__all__ and V.clip_grad_norm_ is O.clip_grad_norm_
    assert callable(O.Adam.clip_grad_norm_)
    ops = import_module(PKG + ".ops")
    assert callable(ops.grad_norm_clip) and callable(ops.adam_apply_clip)


A0, OUT0, WS = 1 << 20, 9 << 20, 10 << 20                            # 16-byte aligned fake device addresses


def _norm_call(lib, g, n, gs, mx, out, ws=WS, count=None, null=()):
    k = len(g)
    arrs = dict(g=(ctypes.c_void_p * k)(*g), n=(ctypes.c_int64 * k)(*n), gs=(ctypes.c_float * k)(*gs),
                mx=(ctypes.c_double * k)(*mx), out=(ctypes.c_void_p * k)(*out))
    for name in null:
        arrs[name] = None
    return lib.vg_grad_norm_clip(arrs["g"], arrs["n"], arrs["gs"], arrs["mx"], k if count is None else count, arrs["out"],
                                 ws, None)


def test_c_abi_rejects_bad_grad_norm_clip_arguments_on_host():
    """Every call here is rejected before a launch: nothing valid is ever passed whole (fake addresses, NULL stream)."""
    lib = import_module(PKG + "._lib").load()
    EINVAL, EALIGN = -1, -2
    ok = dict(g=[A0 + 4], n=[1024], gs=[1.0], mx=[1.0], out=[OUT0])  # valid but for the alignment of g: gets as far as EALIGN

    def call(**kw):
        a = dict(ok)
        extra = {k: kw.pop(k) for k in ("count", "null", "ws") if k in kw}
        a.update(kw)
        return _norm_call(lib, **a, **extra)

    assert call() == EALIGN
    assert call(count=0) == EINVAL and call(count=-1) == EINVAL and call(count=5) == EINVAL
    five = dict(g=[A0] * 5, n=[8] * 5, gs=[1.0] * 5, mx=[1.0] * 5, out=[OUT0] * 5)
    assert _norm_call(lib, **five) == EINVAL
    for name in ("g", "n", "gs", "mx", "out"):
        assert call(null=(name,)) == EINVAL, name
    assert call(ws=None) == EINVAL
    assert call(g=[None]) == EINVAL and call(out=[None]) == EINVAL
    assert call(n=[0]) == EINVAL and call(n=[-4]) == EINVAL
    for m in (float("nan"), -1e-9, -1.0, -INF):
        assert call(mx=[m]) == EINVAL, m
    assert call(mx=[INF]) == EALIGN and call(mx=[0.0]) == EALIGN     # allowed: monitor only / coefficient 0
    for s in (float("nan"), INF, -INF):
        assert call(gs=[s]) == EINVAL, s
    assert call(gs=[-0.5]) == EALIGN and call(gs=[0.0]) == EALIGN
    # the later buffers are checked like the first, and an EINVAL anywhere comes before any EALIGN
    two = dict(g=[A0 + 4, A0 + (1 << 16)], n=[8, 8], gs=[1.0, 1.0], mx=[1.0, float("nan")], out=[OUT0, OUT0 + 8])
    assert _norm_call(lib, **two) == EINVAL
    two.update(mx=[1.0, 1.0], out=[OUT0, None])
    assert _norm_call(lib, **two) == EINVAL
    two.update(out=[OUT0, OUT0 + 8])
    assert _norm_call(lib, **two) == EALIGN
    two.update(g=[A0, A0 + (1 << 16) + 8])
    assert _norm_call(lib, **two) == EALIGN


def _adam_call(lib, p, g, m, v, n, state, coef, count=None, null=()):
    k = len(p)
    vp = lambda xs: (ctypes.c_void_p * k)(*xs)                       # noqa: E731
    arrs = dict(p=vp(p), g=vp(g), m=vp(m), v=vp(v), n=(ctypes.c_int64 * k)(*n), b1=(ctypes.c_double * k)(*[0.9] * k),
                b2=(ctypes.c_double * k)(*[0.999] * k), eps=(ctypes.c_double * k)(*[1e-8] * k),
                gs=(ctypes.c_float * k)(*[1.0] * k), state=vp(state), coef=vp(coef))
    for name in null:
        arrs[name] = None
    return lib.vg_adam_apply_clip(arrs["p"], arrs["g"], arrs["m"], arrs["v"], arrs["n"], arrs["b1"], arrs["b2"], arrs["eps"],
                                  arrs["gs"], arrs["state"], arrs["coef"], k if count is None else count, None)


def test_c_abi_rejects_bad_adam_apply_clip_arguments_on_host():
    lib = import_module(PKG + "._lib").load()
    EINVAL, EALIGN = -1, -2
    P, G_, M, V_, ST, C = (i << 20 for i in range(1, 7))
    ok = dict(p=[P + 4], g=[G_], m=[M], v=[V_], n=[1024], state=[ST], coef=[C])      # gets as far as EALIGN

    def call(**kw):
        a = dict(ok)
        extra = {k: kw.pop(k) for k in ("count", "null") if k in kw}
        a.update(kw)
        return _adam_call(lib, **a, **extra)

    assert call() == EALIGN and call(coef=[None]) == EALIGN          # a NULL coefficient entry is allowed
    assert call(count=0) == EINVAL and call(count=3) == EINVAL and call(count=-1) == EINVAL
    three = dict(p=[P] * 3, g=[G_] * 3, m=[M] * 3, v=[V_] * 3, n=[8] * 3, state=[ST] * 3, coef=[C] * 3)
    assert _adam_call(lib, **three) == EINVAL
    for name in ("p", "g", "m", "v", "n", "b1", "b2", "eps", "gs", "state", "coef"):
        assert call(null=(name,)) == EINVAL, name
    for name in ("p", "g", "m", "v", "state"):
        assert call(**{name: [None]}) == EINVAL, name
    assert call(n=[0]) == EINVAL and call(n=[-1]) == EINVAL
    for name, base in (("g", G_), ("m", M), ("v", V_)):
        assert call(p=[P], **{name: [base + 8]}) == EALIGN, name
    two = dict(p=[P, P + (1 << 16)], g=[G_, G_ + (1 << 16)], m=[M, M + (1 << 16)], v=[V_, V_ + (1 << 16) + 4], n=[8, 8],
               state=[ST, ST + 16], coef=[None, C])
    assert _adam_call(lib, **two) == EALIGN
    two.update(n=[8, 0])
    assert _adam_call(lib, **two) == EINVAL
    two.update(n=[8, 8], state=[ST, None])
    assert _adam_call(lib, **two) == EINVAL


# ---- Python surface ---------------------------------------------------------------------------------------------------
def _fake_adam(O, n=8):
    """An optim.Adam whose flat gradient buffer lives on the CPU (the real constructor needs the device)."""
    o = object.__new__(O.Adam)
    o.flat_g = torch.zeros(n)
    o.clip_dev = o.clip_ws = None
    o._clip_armed = False
    return o


def test_max_grad_norm_validation():
    V = import_module("vaegan_amd")
    O = import_module(PKG + ".optim")
    GC = import_module(PKG + ".gradclip")
    for bad in (float("nan"), -1.0, -INF, "1.0", None, [1.0], True):
        with pytest.raises(ValueError, match="max_norm"):
            O.check_max_norm(bad)
    assert O.check_max_norm(0) == 0.0 and O.check_max_norm(INF) == INF and O.check_max_norm(2) == 2.0
    e, g, d = V.Encoder([3, 64, 64], 100), V.Generator(nz=100, img_size=64), V.Discriminator(img_size=64)
    oe, og, od = (_fake_adam(O) for _ in range(3))
    for bad in (float("nan"), -0.5, "big", [1.0], {"E": float("nan")}, {"E": -1.0}, {"X": 1.0}, {"E": "1"}, {"EG": 1.0}):
        with pytest.raises(ValueError, match="max_norm|max_grad_norm"):
            V.VAEGANTrainer(e, g, d, oe, og, od, max_grad_norm=bad)
    for bad in (float("nan"), -0.5, {"E": 1.0}, {"G": 1.0}):
        with pytest.raises(ValueError, match="max_norm|max_grad_norm"):
            V.VAETrainer(e, g, oe, max_grad_norm=bad)
    for T in (V.DCGANTrainer, V.WGANTrainer):
        for bad in (float("nan"), -0.5, {"E": 1.0}, {"D": -1.0}):
            with pytest.raises(ValueError, match="max_norm|max_grad_norm"):
                T(g, d, og, od, max_grad_norm=bad)
    # off: nothing is allocated and nothing bound; on: one [networks, 2] tensor whose rows are the optimizers' clip_dev
    off = V.VAEGANTrainer(e, g, d, oe, og, od)
    assert off.max_grad_norm is None and off.grad_norms is None and off._clip_key() == () and oe.clip_dev is None
    tr = V.VAEGANTrainer(e, g, d, oe, og, od, max_grad_norm={"G": 2.0, "D": INF})
    assert tr.grad_norms.shape == (3, 2) and oe.clip_dev is None
    assert og.clip_dev.data_ptr() == tr.grad_norms[1].data_ptr() and od.clip_dev.data_ptr() == tr.grad_norms[2].data_ptr()
    assert tr._clip.max == {"G": 2.0, "D": INF} and tr._clip_key()[0][:3] == ("clip", ("G", 2.0), ("D", INF))
    k0 = tr._clip_key()
    tr.max_grad_norm = 3.0                                           # assignable: the same tensor, another key
    assert tr._clip.max == {"E": 3.0, "G": 3.0, "D": 3.0} and tr._clip_key() != k0
    assert tr._clip_key()[0][-1] == k0[0][-1] and oe.clip_dev.data_ptr() == tr.grad_norms[0].data_ptr()
    with pytest.raises(ValueError):
        tr.max_grad_norm = -1.0
    assert tr.max_grad_norm == 3.0                                   # a refused value leaves the option as it was
    tr.max_grad_norm = None
    assert tr.grad_norms is None and tr._clip_key() == ()
    assert isinstance(GC.GradClip(1.0, {"G": og, "D": od}).report(), dict)
    # clip_grad_norm_'s own argument errors come before anything touches a device
    for bad in ([], [oe] * 5, [oe, object()], torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))])):
        with pytest.raises(ValueError, match="vaegan_amd.Adam"):
            V.clip_grad_norm_(bad, 1.0)
    with pytest.raises(ValueError, match="max_norm"):
        V.clip_grad_norm_([oe, og], [1.0])
    with pytest.raises(ValueError, match="max_norm"):
        V.clip_grad_norm_(oe, float("nan"))
