"""GPU: the end of the backward pass below the weight gradients -- the flat Adam step (vg_adam_step, vg_adam_apply after
vg_step_prologue, vg_adam_apply2) against torch.optim.Adam on the CPU and against each other bit for bit, and the operand
pack (vg_pack_weights) against the numpy restatement of the header's formula (tests/_pack_ref.py)."""
import importlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _pack_ref as PR

pytestmark = pytest.mark.gpu

G = PR.G
DEV = "cuda"
LR = 2e-4
BETAS = [((0.5, 0.999), 1e-8), ((0.9, 0.999), 1e-8)]       # the DCGAN trainer's (gan_code.py) and torch's defaults (the VAE-GAN's)
# one workgroup with and without a tail, exactly one float4, whole workgroups + tail, and more float4s than the 2048-workgroup
# cap covers in one pass (the grid-stride loop runs) with a tail
SIZES = [1, 2, 3, 4, 5, 1023, 1024 * 256 + 3, 2048 * 256 * 4 + 4 * 256 * 5 + 2]
STEPS = 4


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module(PR.PKG + ".ops")


def _torch_adam(p0, grads, betas, eps):
    """torch.optim.Adam (single-tensor f32 form) on the CPU -> (p, exp_avg, exp_avg_sq, step)."""
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([p], lr=LR, betas=betas, eps=eps, foreach=False)
    for g in grads:
        p.grad = g.clone()
        opt.step()
    st = opt.state[p]
    return p.detach(), st["exp_avg"], st["exp_avg_sq"], float(st["step"])


def _hip_adam(ops, p0, grads, betas, eps, scale=1.0):
    p = p0.to(DEV)
    m, v, state = torch.zeros_like(p), torch.zeros_like(p), torch.zeros(4, device=DEV)
    for g in grads:
        ops.adam_step(p, g.to(DEV), m, v, LR, betas[0], betas[1], eps, scale, state)
    return p.cpu(), m.cpu(), v.cpu(), float(state[0])


def _compare(got, ref, what):
    """The tolerances of test_adam_against_torch_optim_golden; the largest deviations are printed before they are judged."""
    for name, a, r, atol in (("p", got[0], ref[0], 1e-8), ("exp_avg", got[1], ref[1], 1e-9), ("exp_avg_sq", got[2], ref[2], 1e-12)):
        err = (a.double() - r.double()).abs()
        over = err > atol + 2e-6 * r.double().abs()
        print(f"{what} {name}: max |err| {float(err.max()):.3e}, {int(over.sum())} of {a.numel()} outside rtol 2e-6 atol {atol:g}")
    for name, a, r, atol in (("p", got[0], ref[0], 1e-8), ("exp_avg", got[1], ref[1], 1e-9), ("exp_avg_sq", got[2], ref[2], 1e-12)):
        np.testing.assert_allclose(a.numpy(), r.numpy(), rtol=2e-6, atol=atol, err_msg=f"{what} {name}")
    assert got[3] == ref[3] == STEPS


def _draws(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g), [torch.randn(n, generator=g) for _ in range(STEPS)]


@pytest.mark.parametrize("betas,eps", BETAS, ids=["b0.5", "b0.9"])
@pytest.mark.parametrize("n", SIZES)
def test_adam_step_equals_torch_adam(ops, n, betas, eps):
    p0, grads = _draws(n, n % 1000 + 1)
    _compare(_hip_adam(ops, p0, grads, betas, eps), _torch_adam(p0, grads, betas, eps), f"n={n} betas={betas}")


@pytest.mark.parametrize("scale", [0.125, 1.0 / 3.0], ids=["eighth", "third"])
@pytest.mark.parametrize("n", [5, 1023, 1024 * 256 + 3])
def test_adam_grad_scale_equals_torch_adam_on_scaled_gradients(ops, n, scale):
    """grad_scale (1 / world size under data parallelism): the reference is torch's Adam on g * float32(scale)."""
    betas, eps = BETAS[0]
    p0, grads = _draws(n, n % 1000 + 2)
    ref = _torch_adam(p0, [g * np.float32(scale) for g in grads], betas, eps)
    _compare(_hip_adam(ops, p0, grads, betas, eps, scale), ref, f"n={n} grad_scale={scale:.6f}")


def _optimizer(n, betas, eps, scale, seed):
    """What ops.step_prologue / ops.adam_apply2 read of an optim.Adam: the flat buffers, the device state and the settings."""
    g = torch.Generator().manual_seed(seed)
    return SimpleNamespace(flat_p=torch.randn(n, generator=g).to(DEV), flat_g=torch.zeros(n, device=DEV),
                           exp_avg=torch.zeros(n, device=DEV), exp_avg_sq=torch.zeros(n, device=DEV),
                           state_dev=torch.zeros(4, device=DEV), lr=LR, betas=betas, eps=eps, grad_scale=scale)


def _clone(o):
    return SimpleNamespace(**{k: (v.clone() if torch.is_tensor(v) else v) for k, v in vars(o).items()})


def _fresh_grads(gen, *pairs):
    for a, b in pairs:
        a.flat_g.copy_(torch.randn(a.flat_g.numel(), generator=gen))
        b.flat_g.copy_(a.flat_g)


def _step(ops, o, prepared):
    ops.adam_step(o.flat_p, o.flat_g, o.exp_avg, o.exp_avg_sq, o.lr, o.betas[0], o.betas[1], o.eps, o.grad_scale, o.state_dev,
                  prepared=prepared)


def _assert_same(a, b, what):
    for k in ("flat_p", "exp_avg", "exp_avg_sq", "state_dev"):
        assert torch.equal(getattr(a, k), getattr(b, k)), f"{what}: {k}"


@pytest.mark.parametrize("n", [5, 1023, 1024 * 256 + 3])
def test_prepared_step_equals_plain_step_bit_for_bit(ops, n):
    a = _optimizer(n, (0.5, 0.999), 1e-8, 1.0 / 3.0, 3)
    b = _clone(a)
    gen = torch.Generator().manual_seed(4)
    for it in range(3):
        _fresh_grads(gen, (a, b))
        _step(ops, a, False)
        ops.step_prologue(None, [b])
        _step(ops, b, True)
        _assert_same(a, b, f"step {it + 1}")
    assert float(a.state_dev[0]) == 3.0


@pytest.mark.parametrize("na,nb", [(5, 1023), (1024 * 256 + 3, 7), (2048 * 256 * 4 + 6, 1024 * 256 + 1)])
def test_two_optimizers_in_one_launch_equal_two_launches_bit_for_bit(ops, na, nb):
    """vg_adam_apply2: the boundary between the two buffers (workgroup nb0), the tail of each, the grid-stride loop of the
    first; the buffers differ in betas, eps and grad_scale, so taking a setting from the wrong one shows."""
    a = _optimizer(na, (0.5, 0.999), 1e-8, 0.25, 5)
    b = _optimizer(nb, (0.9, 0.99), 1e-6, 1.0 / 3.0, 6)
    a2, b2 = _clone(a), _clone(b)
    start = a.flat_p.clone()
    gen = torch.Generator().manual_seed(7)
    for it in range(2):
        _fresh_grads(gen, (a, a2), (b, b2))
        ops.step_prologue(None, [a, b])
        ops.adam_apply2(a, b)
        ops.step_prologue(None, [a2, b2])
        _step(ops, a2, True)
        _step(ops, b2, True)
        _assert_same(a, a2, f"first buffer, step {it + 1}")
        _assert_same(b, b2, f"second buffer, step {it + 1}")
    assert float(a.state_dev[0]) == float(b.state_dev[0]) == 2.0 and not torch.equal(a.flat_p, start)


def test_step_prologue_zeroes_the_loss_slots_advances_the_noise_counter_once_and_prepares_the_state(ops):
    noise = ops.NoiseStream(DEV, 1234)
    zero = torch.full((64,), float("nan"), device=DEV)
    a, b = _optimizer(8, (0.5, 0.999), 1e-8, 1.0, 1), _optimizer(8, (0.9, 0.99), 1e-8, 1.0, 2)
    for t in (1, 2, 3):
        zero.fill_(float("nan"))
        ops.step_prologue(noise, [a, b], zero)
        assert torch.equal(zero, torch.zeros(64, device=DEV))
        assert noise.state.tolist() == [1234, t]
        for o in (a, b):
            st = o.state_dev.tolist()
            assert st[0] == float(t) and st[3] == 0.0
            want = np.array([LR / (1.0 - o.betas[0] ** t), np.sqrt(1.0 - o.betas[1] ** t)])
            np.testing.assert_allclose(st[1:3], want, rtol=2.0 ** -23, atol=0)      # f32 of the double value, pow to an ulp
    ops.step_prologue(noise, [])                                                     # the counter alone
    assert noise.state.tolist() == [1234, 4]


# ---- operand pack ------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("dtype", [G.F32, G.BF16], ids=["f32", "bf16"])
def test_pack_weights_equals_the_restated_formula_bit_for_bit(ops, dtype):
    """vg_pack_weights is the reference of vg_pack_weights_multi (test_tiled_multi_pack_equals_reference_pack); this is its
    own: the header's formula in numpy over the same operand list, into a destination pre-filled with NaN bit patterns.
    bf16 is torch's round-to-nearest-even of the f32 value; every padding element (ci >= C, k >= T*IC) is +0."""
    g = torch.Generator().manual_seed(12)
    for pk, wshape in PR.pack_specs(dtype):
        w = torch.randn(wshape, generator=g)
        ref, written = PR.pack_ref(pk, w.numpy())
        out = torch.full((pk.numel(),), float("nan"), device=DEV).to(ops.TORCH_DT[dtype])
        ops.pack_weights(pk, w.to(DEV), dtype, out=out)
        got = out.cpu()
        want = torch.from_numpy(ref).reshape(-1).to(ops.TORCH_DT[dtype])
        assert not torch.isnan(got.float()).any(), pk
        assert torch.equal(_bits(got), _bits(want)), pk
        pad = ~torch.from_numpy(written).reshape(-1)
        assert (_bits(got)[pad] == 0).all(), pk
