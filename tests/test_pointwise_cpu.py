"""CPU: the f64 restatements of tests/_pointwise_ref.py against something independent of them (torch autograd in f64,
torch.nn.functional, the oracle's SSIM), and the input generators of tests/test_gpu_pointwise.py against the conditions
that keep those tests from passing vacuously."""
import pytest
import torch
import torch.nn.functional as F

import _pointwise_ref as R
import vaegan_ref

CLOSE = dict(rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("B,L,MP,ZP", [(6, 100, 200, 100), (3, 100, 208, 104), (5, 7, 16, 8)])
@pytest.mark.parametrize("kl_scale", [0.0, 0.07 / 6])
def test_reparam_kl_backward_is_autograd_through_the_clamp(B, L, MP, ZP, kl_scale):
    mulv, eps, dz = R.reparam_inputs(B, L, MP, ZP, False)
    m = mulv.clone().requires_grad_(True)
    mu, lv = m[:, :L], torch.clamp(m[:, L:2 * L], -10, 10)
    z = mu + torch.exp(0.5 * lv) * eps
    kl_sum = -0.5 * torch.sum(1 + lv - mu.pow(2) - lv.exp())
    ((z * dz[:, :L]).sum() + R.f32(kl_scale) * kl_sum).backward()
    torch.testing.assert_close(R.reparam_kl_backward(mulv, eps, dz, kl_scale, L), m.grad, **CLOSE)
    assert (m.grad[:, 2 * L:] == 0).all()
    z_ref, lv_ref = R.reparam_forward(mulv, eps, L, ZP)
    torch.testing.assert_close(z_ref[:, :L], z.detach(), **CLOSE)
    assert (z_ref[:, L:] == 0).all() and torch.equal(lv_ref, lv.detach())
    torch.testing.assert_close(R.kl_forward(mulv, L, B), kl_sum.detach() / B, **CLOSE)
    assert float(R.kl_abs_terms(mulv, L)) >= abs(float(kl_sum.detach())) * 2


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("C,HW", [(65, 4), (12, 9)])
def test_head_backward_is_autograd_of_bce_sigmoid_conv(groups, C, HW):
    """The weight gradient's layout too: x is NHWC-flattened, dw is [1][C][kh][kw] (HW > 1, C no multiple of 64)."""
    B, k = 7, int(HW ** 0.5)
    g = R.gen(C + groups)
    xi = (torch.randn(groups * B, C, k, k, generator=g, dtype=torch.float64) * 0.5).requires_grad_(True)
    wi = (torch.randn(1, C, k, k, generator=g, dtype=torch.float64) * 0.2).requires_grad_(True)
    p = torch.sigmoid(F.conv2d(xi, wi)).view(-1)
    t0, t1, gscale = 0.9, 0.0, 0.37
    loss = F.binary_cross_entropy(p[:B], torch.full((B,), R.f32(t0), dtype=torch.float64))
    if groups == 2:
        loss = loss + F.binary_cross_entropy(p[B:], torch.full((B,), R.f32(t1), dtype=torch.float64))
    dx, dw = torch.autograd.grad(R.f32(gscale) * loss, (xi, wi))
    x = xi.detach().permute(0, 2, 3, 1).reshape(groups * B, HW * C)
    w = wi.detach().permute(0, 2, 3, 1).reshape(HW * C)
    p_ref, mag = R.dot_sigmoid_forward(x, w)
    torch.testing.assert_close(p_ref, p.detach(), **CLOSE)
    assert (mag >= (x @ w).abs()).all()
    r = R.head_backward(p.detach(), x, w, B, groups, t0, t1, gscale, C, HW)
    torch.testing.assert_close(r["loss"], loss.detach(), **CLOSE)
    torch.testing.assert_close(r["dx"].view(groups * B, k, k, C).permute(0, 3, 1, 2), dx, **CLOSE)
    torch.testing.assert_close(r["dw"].view(1, C, k, k), dw, **CLOSE)
    assert (r["dw_abs"] >= r["dw"].abs()).all()


def test_bce_equals_torch_at_the_log_clamp_and_its_gradient_is_autograd():
    for t in (0.9, 0.0, 1.0):
        p = R.bce_probs(63)
        tt = torch.full_like(p, R.f32(t))
        assert (p == 0).any() and (p == 1).any()
        torch.testing.assert_close(R.bce(p, t), F.binary_cross_entropy(p, tt), **CLOSE)
        for pe in (0.0, 1.0):
            one = torch.tensor([pe], dtype=torch.float64)
            torch.testing.assert_close(R.bce(one, t), F.binary_cross_entropy(one, tt[:1]), **CLOSE)
    p = torch.sigmoid(torch.randn(40, generator=R.gen(2), dtype=torch.float64) * 2).requires_grad_(True)
    (0.37 * F.binary_cross_entropy(p, torch.full_like(p, R.f32(0.9)))).backward()
    torch.testing.assert_close(R.bce_grad(p.detach(), 0.9, 0.37), p.grad * (R.f32(0.37) / 0.37), rtol=1e-11, atol=1e-13)
    # mean loss
    p = torch.randn(33, dtype=torch.float64, generator=R.gen(3)).requires_grad_(True)
    (R.f32(0.37) * -p.mean()).backward()
    torch.testing.assert_close(R.mean_grad(p, -1.0, 0.37), p.grad, **CLOSE)
    torch.testing.assert_close(R.mean_loss(p, -1.0), -p.detach().mean(), **CLOSE)


def test_mse_and_tanh_gradients_are_autograd():
    g = R.gen(4)
    a = torch.randn(2, 3, 5, 7, generator=g, dtype=torch.float64).requires_grad_(True)
    b = torch.randn(2, 3, 5, 7, generator=g, dtype=torch.float64)
    (R.f32(0.37) * F.mse_loss(a, b)).backward()
    torch.testing.assert_close(R.mse_grad(a, b, 0.37), a.grad, **CLOSE)
    torch.testing.assert_close(R.mse(a, b), F.mse_loss(a, b).detach(), **CLOSE)
    # the gradient through tanh, with and without the second branch that already sits in NHWC
    pre = torch.randn(2, 3, 5, 7, generator=g, dtype=torch.float64).requires_grad_(True)
    t = torch.tanh(pre)
    dy = torch.randn(2, 3, 5, 7, generator=g, dtype=torch.float64)
    add = torch.randn(2, 3, 5, 7, generator=g, dtype=torch.float64)
    (gp,) = torch.autograd.grad(t, pre, dy, retain_graph=True)
    got = R.nchw_grad_to_nhwc(dy, 8, tanh_out=t.detach())
    torch.testing.assert_close(R.from_nhwc(got, 3), gp, **CLOSE)
    assert (got[..., 3:] == 0).all()
    (gp2,) = torch.autograd.grad(t, pre, dy + add)
    got = R.nchw_grad_to_nhwc(dy, 8, tanh_out=t.detach(), add_nhwc=R.to_nhwc(add, 8))
    torch.testing.assert_close(R.from_nhwc(got, 3), gp2, **CLOSE)
    y, yn = R.nhwc_tanh_to_nchw_noisy(R.to_nhwc(pre.detach(), 4), 3, dy, 0.05)
    torch.testing.assert_close(y, t.detach(), **CLOSE)
    torch.testing.assert_close(R.from_nhwc(yn, 3), t.detach() + R.f32(0.05) * dy, **CLOSE)
    # activation backward
    x, gy = R.act_inputs(4 * 333, False)
    xr = x.clone().requires_grad_(True)
    for act, slope, fn in ((1, 0.0, F.relu), (2, 0.2, lambda v: F.leaky_relu(v, R.f32(0.2)))):
        (gx,) = torch.autograd.grad(fn(xr), xr, gy)
        torch.testing.assert_close(R.act_backward(x, gy, act, slope), gx, **CLOSE)


@pytest.mark.parametrize("kind", R.SSIM_KINDS)
@pytest.mark.parametrize("B,C,H,W", [(1, 1, 11, 11), (2, 3, 12, 17), (2, 3, 64, 64)])
def test_ssim_window_form_equals_the_oracle_conv_form(kind, B, C, H, W):
    a, b = R.ssim_inputs(kind, B, C, H, W)
    assert abs(R.ssim(a, b) - vaegan_ref.ssim((a.double() + 1) / 2, (b.double() + 1) / 2)) <= 1e-12
    if kind == "same":
        assert abs(R.ssim(a, b) - 1.0) <= 1e-12
    if kind == "small_noise":
        assert 0.3 < R.ssim(a, b) < 0.95


def test_unit_roundoff_of_the_storage_formats():
    """The output-rounding terms of the GPU bounds: round-to-nearest to bf16 errs by up to 2^-8 |x| (8 significant bits;
    half that, 2^-9 |x|, is exceeded by the correctly rounded conversion itself), to f32 by up to 2^-24 |x|."""
    x = torch.rand(1 << 16, generator=R.gen(0), dtype=torch.float64) + 1.0
    rel = ((x.to(torch.bfloat16).double() - x).abs() / x)
    assert float(rel.max()) <= R.UB and float(rel.max()) > 2.0 ** -9
    assert float(((x.float().double() - x).abs() / x).max()) <= R.U


# ---- the generators' conditions -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("B,L,MP,ZP", [(6, 100, 200, 100), (3, 100, 208, 104), (5, 7, 16, 8), (41, 100, 200, 104),
                                       (128, 100, 200, 104)])
def test_reparam_inputs_leave_and_touch_the_clamp(B, L, MP, ZP, bf16):
    mulv, _, _ = R.reparam_inputs(B, L, MP, ZP, bf16)
    lv = mulv[:, L:2 * L]
    frac = float(((lv < -10) | (lv > 10)).double().mean())
    assert 0.10 <= frac <= 0.60, frac
    assert (lv == 10).any() or (lv == -10).any()
    if B * L >= 4:
        assert (lv == 10).any() and (lv == -10).any()


@pytest.mark.parametrize("B,C,H,W", [(3, 3, 10, 10), (2, 3, 5, 7), (2, 1, 6, 6), (2, 4, 4, 4), (1, 3, 64, 64)])
def test_noisy_clamp_inputs_sit_on_both_bounds(B, C, H, W):
    x, eps, sigma = R.noisy_clamp_inputs(B, C, H, W)
    _, v = R.noisy_clamp_to_nhwc(x, eps, sigma, -1.0, 1.0, 4)
    for bound in (-1.0, 1.0):
        frac = float((v == bound).double().mean())
        assert 0.10 <= frac <= 0.60, (bound, frac)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("n", [4, 4 * 333])
def test_activation_inputs_cover_both_branches_away_from_zero(n, bf16):
    x, _ = R.act_inputs(n, bf16)
    assert float((x > 0).double().mean()) >= 0.25 and float((x < 0).double().mean()) >= 0.25
    assert float(x.abs().min()) >= 1e-3


def test_bce_probs_hold_the_edges():
    for B in (1, 63, 256, 257, 1000):
        p = R.bce_probs(B)
        assert p.numel() == B and (p >= 0).all() and (p <= 1).all() and torch.equal(p, p.float().double())
        if B >= 6:
            assert (p == 0).any() and (p == 1).any()
            assert ((p > 0) & (p <= 1e-7)).any() and ((p < 1) & (p >= 1 - 1e-7)).any()
