"""No GPU: the restatement the augmentation kernels are tested against (tests/_diffaug_ref.py) is itself checked -- against the
sequential brightness -> saturation -> contrast -> translation -> cutout form, against torch autograd in f64, through the
adjoint identity and at the edges of the mask and the shift -- and the exactness of the inputs the GPU tests compare bit for
bit, the host-side argument checks of every entry point, policy parsing, the oracle's iteration under the identity table and
the exported symbols against the built library and package."""
import os
import re
from importlib import import_module

import numpy as np
import pytest
import torch

import _diffaug_ref as DR
import siblings_ref as SR
import vaegan_ref as R
from _inputs import make_inputs
from vaegan_amd import DiffAugment  # noqa: F401  (this file is about the feature: without it nothing here is collected)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
F32, F64 = np.float32, np.float64
SHAPES = [(2, 2, 2, 3), (4, 8, 8, 3), (3, 10, 6, 1), (4, 16, 16, 4), (2, 40, 40, 3)]      # the last: two parts per image


random_table, exact_case = DR.random_table, DR.exact_case


# ---- the restatement against the sequential form and autograd ---------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_f64_restatement_forward_equals_the_sequential_form(shape):
    N, H, W, C = shape
    rng = np.random.default_rng(sum(shape))
    worst = 0.0
    for PB in (N, max(1, N // 2)) if N % 2 == 0 else (N,):
        x = rng.standard_normal(shape)
        t = random_table(rng, PB, H, W)
        cut = (DR.cut_size(H), DR.cut_size(W))
        got = DR.forward(x, t, *cut, dt=F64)
        xt = torch.from_numpy(x).permute(0, 3, 1, 2)
        seq = DR.torch_sequential(xt, t, *cut).permute(0, 2, 3, 1).numpy()
        closed = DR.torch_closed(xt, t, *cut).permute(0, 2, 3, 1).numpy()
        worst = max(worst, float(np.abs(got - seq).max()), float(np.abs(got - closed).max()))
        np.testing.assert_allclose(got, seq, rtol=0, atol=1e-14)
        np.testing.assert_allclose(got, closed, rtol=0, atol=1e-14)
    print(f"{shape}: closed form against the sequential form, worst absolute difference {worst:.2e}")


@pytest.mark.parametrize("shape", SHAPES)
def test_f64_restatement_backward_equals_torch_autograd(shape):
    N, H, W, C = shape
    rng = np.random.default_rng(7 + sum(shape))
    x = rng.standard_normal(shape)
    g = rng.standard_normal(shape)
    t = random_table(rng, N, H, W)
    cut = (DR.cut_size(H), DR.cut_size(W))
    xt = torch.from_numpy(x).permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = DR.torch_sequential(xt, t, *cut)
    (y * torch.from_numpy(g).permute(0, 3, 1, 2)).sum().backward()
    want = xt.grad.permute(0, 2, 3, 1).numpy()
    got = DR.backward(g, t, *cut, dt=F64)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-14)


@pytest.mark.parametrize("shape", SHAPES)
def test_adjoint_identity_in_f64(shape):
    """<T x, g> = <x, T' g> for the linear part (beta = 0)."""
    N, H, W, C = shape
    rng = np.random.default_rng(11 + sum(shape))
    x, g = rng.standard_normal(shape), rng.standard_normal(shape)
    t = random_table(rng, N, H, W)
    t[:, 0] = 0.0
    cut = (DR.cut_size(H), DR.cut_size(W))
    lhs = float((DR.forward(x, t, *cut, dt=F64) * g).sum())
    rhs = float((x * DR.backward(g, t, *cut, dt=F64)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))


def test_exact_inputs_are_exact():
    """The inputs of the GPU tests' bitwise comparison: the f32 restatement equals the f64 one on them, forward and backward,
    so no order of summation and no contraction can hide -- and every value survives bf16 storage of the INPUT (the result
    is compared after one rounding to bf16 on both sides)."""
    for (N, H, W, C) in [(2, 2, 2, 3), (4, 8, 8, 3), (4, 16, 16, 4), (8, 64, 64, 3)]:
        for PB in (N, N // 2):
            x, t = exact_case(N, H, W, C, PB, 100 + H + PB)
            assert np.array_equal(DR.from_bf16(DR.to_bf16(x)), x)
            cut = (DR.cut_size(H), DR.cut_size(W))
            for fn in (DR.forward, DR.backward):
                a32, a64 = fn(x, t, *cut, dt=F32), fn(x, t, *cut, dt=F64)
                assert a32.dtype == F32 and np.array_equal(a32.astype(F64), a64), (fn.__name__, N, H, W, C, PB)


# ---- edges of the mask and the shift ----------------------------------------------------------------------------------
def test_shift_edges():
    H, W = 5, 4
    x = np.arange(1, H * W + 1, dtype=F64).reshape(1, H, W, 1)
    for ty, tx in [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1), (H - 1, 0), (-(H - 1), 0), (0, W - 1), (0, -(W - 1)), (2, -3)]:
        t = DR.identity_table(1)
        t[0, 3], t[0, 4] = ty, tx
        y = DR.forward(x, t, 0, 0, dt=F64)[0, :, :, 0]
        for h in range(H):
            for w in range(W):
                inside = 0 <= h + ty < H and 0 <= w + tx < W
                assert y[h, w] == (x[0, h + ty, w + tx, 0] if inside else 0.0)
    for ty, tx in [(H, 0), (-H, 0), (0, W), (0, -W), (1000, 1000)]:
        t = DR.identity_table(1)
        t[0, 3], t[0, 4] = ty, tx
        assert not DR.forward(x, t, 0, 0, dt=F64).any()
        assert not DR.backward(x, t, 0, 0, dt=F64).any()


def test_cutout_edges_and_bad_entries():
    H, W = 6, 6
    x = np.ones((1, H, W, 1))
    t = DR.identity_table(1)
    for cy, cx, zeros in [(-10, -10, 0), (H, 0, 0), (0, W, 0), (-1, -1, 4), (4, 4, 4), (0, 0, 9), (-3, 2, 0), (-2, 5, 1)]:
        t[0, 5], t[0, 6] = cy, cx
        y = DR.forward(x, t, 3, 3, dt=F64)
        assert int((y == 0).sum()) == zeros, (cy, cx)
    t[0, 5], t[0, 6] = 0, 0
    assert not DR.forward(x, t, H, W, dt=F64).any()                  # covers everything
    assert DR.forward(x, t, 0, 3, dt=F64).all() and DR.forward(x, t, 3, 0, dt=F64).all()
    # NaN / huge: a shift counts as 0, a cutout origin as "no cutout"
    for bad in (np.nan, 1e30, -1e30, 2.0 ** 30):
        for slot in (3, 4):
            t = DR.identity_table(1)
            t[0, slot] = bad
            assert np.array_equal(DR.forward(x, t, 0, 0, dt=F64), x)
        for slot in (5, 6):
            t = DR.identity_table(1)
            t[0, slot] = bad
            assert np.array_equal(DR.forward(x, t, 3, 3, dt=F64), x)
            assert np.array_equal(DR.backward(x, t, 3, 3, dt=F64), x)


def test_identity_row_and_row_sharing():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((4, 8, 8, 3)).astype(F32)
    assert np.array_equal(DR.forward(x, DR.identity_table(2), 0, 0), x)
    assert np.array_equal(DR.backward(x, DR.identity_table(4), 0, 0), x)
    t = random_table(rng, 2, 8, 8)
    y = DR.forward(x, t, 4, 4)
    assert np.array_equal(y[2:], DR.forward(x[2:], t, 4, 4))        # image n uses row n % PB


def test_params_restatement_ranges_and_identity_bits():
    rng = np.random.default_rng(9)
    H, W = 64, 48
    u24 = rng.integers(0, 1 << 24, (4096, 8))
    u24[0], u24[1] = 0, (1 << 24) - 1                                # both ends of every range
    p = DR.params_from_u24(u24, 31, H, W)
    assert p.dtype == F32 and p.shape == (4096, 8) and not p[:, 7].any()
    assert p[:, 0].min() == -0.5 and p[:, 0].max() < 0.5 and p[:, 1].min() == 0 and p[:, 1].max() < 2
    assert p[:, 2].min() == 0.5 and p[:, 2].max() <= 1.5
    assert (p[0, 3], p[1, 3], p[0, 4], p[1, 4]) == (-8, 8, -6, 6)
    assert (p[0, 5], p[1, 5], p[0, 6], p[1, 6]) == (-16, 48, -12, 36)
    assert np.array_equal(p[:, 3:7], np.round(p[:, 3:7]))
    for bit, cols, ident in ((1, [0], 0.0), (2, [1], 1.0), (4, [2], 1.0), (8, [3, 4], 0.0), (16, [5, 6], 0.0)):
        q = DR.params_from_u24(u24, 31 & ~bit, H, W)
        assert (q[:, cols] == ident).all()
        keep = [c for c in range(8) if c not in cols]
        assert np.array_equal(q[:, keep], p[:, keep])
    assert np.array_equal(DR.params_from_u24(u24, 0, H, W), DR.identity_table(4096))
    # an odd size: the cutout offset's range loses its upper end
    p = DR.params_from_u24(u24[:2], 16, 5, 5)
    assert DR.cut_size(5) == 3 and (p[0, 5], p[1, 5]) == (-1, 3)


# ---- policy parsing and the public surface ----------------------------------------------------------------------------
def test_policy_parsing():
    A = import_module(PKG + ".augment")
    assert A.parse_policy("color,translation,cutout") == 31 == DiffAugment().bits
    assert A.parse_policy("color") == 7 and A.parse_policy("brightness, contrast") == 5
    assert A.parse_policy("") == 0 and A.parse_policy("cutout,cutout") == 16
    for bad in ("colour", "color;cutout", "flip"):
        with pytest.raises(ValueError):
            DiffAugment(bad)
    with pytest.raises(ValueError):
        A.parse_policy(None)
    a = DiffAugment("translation")
    assert A.DiffAugment.of(a) is a and A.DiffAugment.of(None) is None and A.DiffAugment.of("color").bits == 7
    assert a.key() != DiffAugment("color").key() and not a.need_sum and DiffAugment("contrast").need_sum
    ops = import_module(PKG + ".ops")
    assert ops.diffaug_cut(31, 64, 33) == (32, 17) == DR.cut_of(31, 64, 33) and ops.diffaug_cut(15, 64, 64) == (0, 0)


def test_new_symbols_are_exported_and_the_abi_version_moved():
    L = import_module(PKG + "._lib")
    lib = L.load()
    src = open(os.path.join(ROOT, "include", "vaegan_hip.h")).read()
    assert int(re.search(r"#define\s+VG_ABI_VERSION\s+(\d+)", src).group(1)) == L.ABI_VERSION >= 25
    assert lib.vg_abi_version() == L.ABI_VERSION
    for name in ("vg_diffaug_params", "vg_diffaug_forward", "vg_diffaug_backward", "vg_diffaug_ws_floats"):
        assert name in L.SIGNATURES and name in src and getattr(lib, name) is not None
    ops = import_module(PKG + ".ops")
    assert int(re.search(r"#define\s+VG_DRAW_AUGMENT\s+(\d+)", src).group(1)) == ops.DRAW_AUGMENT == 48
    V = import_module("vaegan_amd")
    assert "DiffAugment" in V.__all__ and V.DiffAugment is import_module(PKG + ".augment").DiffAugment
    for fn in ("diffaug_params", "diffaug_forward", "diffaug_backward"):
        assert callable(getattr(ops, fn))


# ---- C ABI on the host ------------------------------------------------------------------------------------------------
EINVAL, EALIGN, ENOSUP = -1, -2, -3
A0, OUT0, P0, WS0 = 1 << 20, 9 << 20, 17 << 20, 18 << 20             # 16-byte aligned fake device addresses


@pytest.mark.parametrize("name", ["vg_diffaug_forward", "vg_diffaug_backward"])
def test_apply_entry_points_check_their_arguments_on_the_host(name):
    """Every rejection happens before a launch: no GPU is needed (and none is touched) to see the codes."""
    L = import_module(PKG + "._lib")
    fn = getattr(L.load(), name)

    def call(inp=A0, out=OUT0, params=P0, N=4, PB=2, H=8, W=8, C=3, CP=8, cut_h=4, cut_w=4, ws=WS0, cap=4, dtype=L.VG_BF16):
        return fn(inp, out, params, N, PB, H, W, C, CP, cut_h, cut_w, ws, cap, dtype, None)

    for kw in (dict(inp=None), dict(out=None), dict(params=None), dict(out=A0), dict(PB=3), dict(PB=0), dict(N=0), dict(H=0),
               dict(W=0), dict(C=0), dict(C=9), dict(cap=3), dict(cut_h=-1), dict(cut_w=9), dict(H=1 << 15, W=1 << 15, cap=1 << 40)):
        assert call(**kw) == EINVAL, kw
    for kw in (dict(inp=A0 + 8), dict(out=OUT0 + 4), dict(params=P0 + 8), dict(ws=WS0 + 4), dict(CP=4), dict(CP=12),
               dict(dtype=L.VG_F32, CP=6, C=3)):
        assert call(**kw) == EALIGN, kw
    for kw in (dict(dtype=L.VG_FP8), dict(dtype=7)):
        assert call(**kw) == ENOSUP, kw
    assert lib_ws(L)(4, 8, 8) == 4 and lib_ws(L)(2, 64, 64) == 8 and lib_ws(L)(3, 33, 31) == 3
    for bad in ((0, 8, 8), (4, 0, 8), (4, 8, 0), (1, 1 << 15, 1 << 15)):
        assert lib_ws(L)(*bad) == EINVAL


def lib_ws(L):
    return L.load().vg_diffaug_ws_floats


def test_params_entry_point_checks_its_arguments_on_the_host():
    L = import_module(PKG + "._lib")
    fn = L.load().vg_diffaug_params
    for args in ((None, 4, 31, 8, 8, OUT0), (A0, 4, 31, 8, 8, None), (A0, 0, 31, 8, 8, OUT0), (A0, 4, 32, 8, 8, OUT0),
                 (A0, 4, -1, 8, 8, OUT0), (A0, 4, 31, 0, 8, OUT0), (A0, 4, 31, 8, 0, OUT0), (A0, 4, 31, 1 << 24, 8, OUT0)):
        assert fn(*args, None) == EINVAL, args


def test_wrappers_reject_host_tensors_and_bad_shapes():
    ops = import_module(PKG + ".ops")
    x = torch.zeros(2, 4, 4, 4)
    p = torch.zeros(2, 8)
    with pytest.raises(RuntimeError):
        ops.diffaug_forward(x, p, 3, (0, 0), 0)
    with pytest.raises(RuntimeError):
        ops.diffaug_backward(x, p, 3, (0, 0), 0)
    with pytest.raises(RuntimeError):
        ops.diffaug_params(torch.zeros(2, dtype=torch.int64), 2, 31, 4, 4)


# ---- the oracle's iteration -------------------------------------------------------------------------------------------
S, B = 64, 4


def _state(m):
    out = []
    for st in (m.E, m.G, m.D):
        out += [st[k].detach().clone() for k in sorted(st)]
    return out


def test_ref_step_with_the_identity_table_is_the_oracles_own_step():
    real, ez, er, ec = make_inputs(B, S, 7000)
    own = R.RefVAEGAN(img_size=S)
    want = own.train_step(real, ez, er, ec, 60)
    for table, cut in ((None, (0, 0)), (DR.identity_table(B), (0, 0)), (DR.identity_table(B), (0, 32))):
        m = R.RefVAEGAN(img_size=S)
        got = DR.ref_step(m, real, ez, er, ec, 60, table, cut)
        for k, v in want.items():
            assert got[k] == v, k
        for a, b in zip(_state(own), _state(m)):
            assert torch.equal(a, b)
    # a real table changes what D sees, not the reconstruction's forward
    rng = np.random.default_rng(1)
    m = R.RefVAEGAN(img_size=S)
    got = DR.ref_step(m, real, ez, er, ec, 60, random_table(rng, B, S, S), (32, 32))
    assert got["recon_loss"] == want["recon_loss"] and got["kl_loss"] == want["kl_loss"]
    assert got["d_loss_1"] != want["d_loss_1"] and got["g_loss_adv"] != want["g_loss_adv"]


def test_sibling_ref_steps_with_the_identity_table_are_the_oracles_own_steps():
    g = torch.Generator().manual_seed(8100)
    real = torch.rand(B, 3, S, S, generator=g) * 2 - 1
    noises = [torch.randn(B, 100, 1, 1, generator=g) for _ in range(3)]
    own, m = SR.RefDCGAN(img_size=S), SR.RefDCGAN(img_size=S)
    assert own.train_step(real, noises[0]) == DR.ref_dcgan_step(m, real, noises[0], DR.identity_table(B))
    for k in own.D:
        assert torch.equal(own.D[k], m.D[k]), k
    own, m = SR.RefWGAN(img_size=S), SR.RefWGAN(img_size=S)
    assert own.train_step(real, noises[:2], noises[2]) == DR.ref_wgan_step(m, real, noises[:2], noises[2], DR.identity_table(B))
    for k in own.G:
        assert torch.equal(own.G[k], m.G[k]), k
