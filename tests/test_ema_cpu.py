"""No GPU: the restatement the weight-averaging kernel is tested against (tests/_ema_ref.py) is itself checked -- against
torch's AveragedModel in f64, against the closed form of a constant target, at the warm-up crossings -- and the exported
symbol, the host-side argument checks of vg_ema_update and the argument errors of vaegan_amd.EMA against the built library."""
import ctypes
import os
import re
from importlib import import_module

import numpy as np
import pytest
import torch
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

import _ema_ref as ER
from vaegan_amd import EMA  # noqa: F401  (this file is about the feature: without it nothing here is collected)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
F32 = np.float32


def test_f64_restatement_equals_torch_averaged_model():
    """Constant decay, f64: AveragedModel's first update_parameters copies, every later one is lerp(ema, p, 1 - decay) =
    ema + (1 - decay) (p - ema) for a weight below 0.5 -- the contract's formula in double.  Exact on the machines seen;
    held to 2^-50 relative."""
    decay, steps = 0.9, 39
    g = torch.Generator().manual_seed(11)
    model = torch.nn.Linear(7, 5).double()
    avg = AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(decay))
    avg.update_parameters(model)                                  # the copy
    mine = [p.detach().numpy().copy() for p in model.parameters()]
    worst = 0.0
    for t in range(1, steps + 1):
        with torch.no_grad():
            for p in model.parameters():
                p.add_(torch.randn(p.shape, generator=g, dtype=torch.float64) * 0.1)
        avg.update_parameters(model)
        mine = [ER.step_f64(e, p.detach().numpy(), decay, False, t) for e, p in zip(mine, model.parameters())]
        for e, q in zip(mine, avg.module.parameters()):
            q = q.detach().numpy()
            worst = max(worst, float(np.abs(e - q).max() / np.abs(q).max()))
    print(f"f64 restatement against AveragedModel over {steps} steps: worst relative difference {worst:.3e}")
    assert worst <= 2.0 ** -50


def test_warmup_values_and_crossings():
    assert ER.decay_f32(0.999, True, 1) == F32(2.0 / 11.0)
    assert ER.decay_f32(0.999, False, 1) == F32(0.999)
    # decay 0.5: (1 + t) / (10 + t) reaches 0.5 at t = 8 (9 / 18), below it the ramp holds
    assert ER.decay_f64(0.5, True, 7) == 8.0 / 17.0 < 0.5 and ER.decay_f32(0.5, True, 7) == F32(8.0 / 17.0)
    assert ER.decay_f64(0.5, True, 8) == 0.5 and ER.decay_f64(0.5, True, 9) == 0.5
    assert ER.weight_f32(0.5, True, 8) == F32(0.5) and ER.weight_f32(0.5, True, 7) == F32(1) - F32(8.0 / 17.0)
    # decay 0.999: the cap takes over at t = 8990 (8991 / 9000 = 0.999); 8989 (8990 / 8999) is still on the ramp
    assert ER.decay_f64(0.999, True, 8989) == 8990.0 / 8999.0 < 0.999
    assert ER.decay_f32(0.999, True, 8989) == F32(8990.0 / 8999.0) != F32(0.999)
    assert ER.decay_f32(0.999, True, 8990) == F32(0.999) and ER.decay_f32(0.999, True, 8991) == F32(0.999)
    assert ER.decay_f32(0.999, True, 10 ** 6) == F32(0.999)
    # t travels as an f32 (state[0]): every value used here is an integer below 2^24, exact
    assert float(F32(8990)) == 8990.0


def test_f32_restatement_against_the_closed_form_of_a_constant_target():
    """p constant, weight w constant: exactly, x_t = e_t - p obeys x_{t+1} = (1 - w) x_t, i.e. e_T = p + (1 - w)^T (e_0 - p).
    One f32 step computes e' = (e + w (p - e) (1 + a)(1 + b)) (1 + c) with |a|, |b|, |c| <= u = 2^-24 (subtraction, product,
    sum), so its x' = (1 - w) x - w x ((1 + a)(1 + b) - 1) + c e': the step adds at most  w |x| (2u + u^2) + u |e'|  to the
    error, and what was there before shrinks by (1 - w).  |x| never grows past X = |e_0 - p| and e' stays between e_0 and
    p, so |e'| <= M = max(|e_0|, |p|) (each up to a factor 1 + O(T u), which the 1.01 below covers), hence
        |error_T| <= sum_t (1 - w)^(T - t) u (2 w X + M) <= min(T, 1 / w) u (2 w X + M).
    The closed form is evaluated in f64 with the f32 weight the kernel uses.  Observed over 200 steps at decay 0.9 on
    values of magnitude up to 16: 3.8e-6 absolute (2.4e-7 of the largest value), 0.78 of the elementwise bound at worst; the
    bound itself reaches 10 * 2^-24 * (0.2 * 32 + 16) = 1.3e-5."""
    decay, T = 0.9, 200
    e0, p = ER.inputs(4096, 5)
    w = ER.weight_f32(decay, False, 0)
    ER.check_conditions(e0, p, w)
    e = e0.copy()
    for t in range(1, T + 1):
        e = ER.step_f32(e, p, decay, False, t)
    w64 = float(w)
    closed = p.astype(np.float64) + (1.0 - w64) ** T * (e0.astype(np.float64) - p.astype(np.float64))
    u = 2.0 ** -24
    X = np.abs(e0.astype(np.float64) - p.astype(np.float64))
    M = np.maximum(np.abs(e0), np.abs(p)).astype(np.float64)
    bound = 1.01 * min(T, 1.0 / w64) * u * (2.0 * w64 * X + M)
    err = np.abs(e.astype(np.float64) - closed)
    print(f"f32 restatement against the closed form, {T} steps at decay {decay}: max error {err.max():.3e}, "
          f"largest error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all()


def test_decay_one_leaves_finite_inputs_bitwise_unchanged():
    """w = 0: e + 0 * (p - e) = e + (+-0) = e for every finite e, p (a zero e keeps its sign: -0 + -0 = -0, -0 + +0 would
    be +0, but 0 * (p - e) with e = -0 has the sign of p, so only e = +0 is generated here).  decay = 0 (w = 1) is NOT the
    identity onto p: e + (p - e) rounds twice."""
    e0, p = ER.inputs(4096, 6)
    out = ER.step_f32(e0, p, 1.0, False, 3)
    assert np.array_equal(out.view(np.int32), e0.view(np.int32))
    out = ER.step_f32(e0, p, 1.0, True, 10 ** 9)                  # the ramp has reached the cap: (1 + t) / (10 + t) rounds to 1
    assert ER.weight_f32(1.0, True, 10 ** 9) == 0 and np.array_equal(out.view(np.int32), e0.view(np.int32))
    once = ER.step_f32(e0, p, 0.0, False, 1)
    assert not np.array_equal(once, p)                            # documented, not a defect


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_input_generator_meets_the_conditions_the_gpu_tests_rely_on(seed):
    e, p = ER.inputs(1 << 16, seed)
    assert (e == 0).any() and (p == 0).any() and np.signbit(p[p == 0]).any() and not np.signbit(e[e == 0]).any()
    for decay, warmup, t in ((0.999, True, 1), (0.5, True, 7), (0.5, True, 8), (0.999, True, 8989), (0.999, True, 8990),
                             (0.9, False, 0), (1.0, False, 0), (0.0, False, 0), (0.9999, False, 0)):
        w = ER.weight_f32(decay, warmup, t)
        ER.check_conditions(e, p, w)
        x = e
        for _ in range(3):                                        # the results of an update are inputs of the next
            x = ER.step_f32(x, p, decay, warmup, t)
        nz = np.abs(x[x != 0])
        assert nz.min() >= np.finfo(F32).tiny


def test_same_bits_matches_nan_positions():
    a = np.array([1.0, np.nan, -0.0], dtype=F32)
    assert ER.same_bits(a.copy(), a)
    assert not ER.same_bits(np.array([1.0, np.nan, 0.0], dtype=F32), a)
    assert not ER.same_bits(np.array([1.0, 2.0, -0.0], dtype=F32), a)
    assert not ER.same_bits(np.array([np.nan, np.nan, -0.0], dtype=F32), a)


def test_new_symbol_is_exported_and_the_abi_version_moved():
    L = import_module(PKG + "._lib")
    lib = L.load()
    src = open(os.path.join(ROOT, "include", "vaegan_hip.h")).read()
    assert int(re.search(r"#define\s+VG_ABI_VERSION\s+(\d+)", src).group(1)) == L.ABI_VERSION >= 22
    assert lib.vg_abi_version() == L.ABI_VERSION
    assert "vg_ema_update" in L.SIGNATURES and "vg_ema_update" in src and "Weight averaging" in src
    assert getattr(lib, "vg_ema_update") is not None
    assert int(re.search(r"#define\s+VG_EMA_MAX\s+(\d+)", src).group(1)) == L.VG_EMA_MAX == 4
    V = import_module("vaegan_amd")
    assert "EMA" in V.__all__ and V.EMA is import_module(PKG + ".ema").EMA
    assert callable(import_module(PKG + ".ops").ema_update)


def _call(lib, ema, p, n, state, decay, warmup, count=None, null=()):
    """vg_ema_update on host arrays of FAKE device addresses (nothing valid is ever passed whole: every call is rejected
    before a launch).  null: names of the arrays passed as NULL."""
    k = len(ema)
    arrs = dict(ema=(ctypes.c_void_p * k)(*ema), p=(ctypes.c_void_p * k)(*p), n=(ctypes.c_int64 * k)(*n),
                state=(ctypes.c_void_p * k)(*state), decay=(ctypes.c_double * k)(*decay), warmup=(ctypes.c_int * k)(*warmup))
    for name in null:
        arrs[name] = None
    return lib.vg_ema_update(arrs["ema"], arrs["p"], arrs["n"], arrs["state"], arrs["decay"], arrs["warmup"],
                             k if count is None else count, None)


def test_c_abi_rejects_bad_ema_arguments_on_host():
    """Validation happens before any launch (pattern: test_ssimloss_cpu.test_c_abi_rejects_bad_ssim_loss_arguments_on_host)."""
    lib = import_module(PKG + "._lib").load()
    EINVAL, EALIGN = -1, -2
    E, P, S, N = 1 << 20, 2 << 20, 3 << 20, 1024                   # disjoint, 16-byte aligned fake addresses
    ok = dict(ema=[E], p=[P], n=[N], state=[S], decay=[0.999], warmup=[1])

    def bad(**kw):
        a = dict(ok)
        extra = {k: kw.pop(k) for k in ("count", "null") if k in kw}
        a.update(kw)
        return _call(lib, **a, **extra)

    assert bad(count=0) == EINVAL and bad(count=-1) == EINVAL and bad(count=5) == EINVAL
    five = dict(ema=[E] * 5, p=[P] * 5, n=[N] * 5, state=[S] * 5, decay=[0.5] * 5, warmup=[0] * 5)
    assert _call(lib, **five) == EINVAL
    for name in ("ema", "p", "n", "state", "decay", "warmup"):
        assert bad(null=(name,)) == EINVAL, name                    # a NULL array
    assert bad(ema=[None]) == EINVAL and bad(p=[None]) == EINVAL    # a NULL entry
    assert bad(state=[None]) == EINVAL                              # warmup set with a NULL state
    assert bad(n=[0]) == EINVAL and bad(n=[-4]) == EINVAL
    for d in (float("nan"), float("inf"), -float("inf"), -1e-9, 1.0 + 1e-9, 2.0):
        assert bad(decay=[d]) == EINVAL, d
    assert bad(p=[E]) == EINVAL                                     # the same range
    assert bad(p=[E + 4 * (N - 1)]) == EINVAL and bad(p=[E - 4 * (N - 1)]) == EINVAL      # one element shared, either side
    assert bad(ema=[E + 4]) == EALIGN and bad(p=[P + 8]) == EALIGN  # valid but for the 16-byte contract
    assert bad(ema=[E + 4], state=[None], warmup=[0]) == EALIGN     # ... a NULL state without warm-up is accepted that far
    # the second buffer is checked like the first, and an EINVAL anywhere comes before any EALIGN
    two = dict(ema=[E, E + (8 << 20)], p=[P, P + (8 << 20)], n=[N, N], state=[S, None], decay=[0.9, 0.9], warmup=[1, 1])
    assert _call(lib, **two) == EINVAL
    two.update(warmup=[1, 0], ema=[E + 4, E + (8 << 20)], decay=[0.9, 1.5])
    assert _call(lib, **two) == EINVAL
    two.update(decay=[0.9, 0.9])
    assert _call(lib, **two) == EALIGN


def test_ema_argument_errors():
    V = import_module("vaegan_amd")
    O = import_module(PKG + ".optim")
    for d in (-0.1, 1.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="decay"):
            V.EMA([], [], decay=d)
    with pytest.raises(ValueError, match="at least one module"):
        V.EMA([], [])
    g = V.Generator(nz=16, ngf=16, img_size=16)
    h = V.Generator(nz=16, ngf=16, img_size=16)

    def fake_adam(params):
        """An optim.Adam whose flat buffer lives on the CPU (the real constructor needs the device): homes `params`."""
        o = object.__new__(O.Adam)
        o.params = list(params)
        o.offsets, n = [], 0
        for q in o.params:
            o.offsets.append(n)
            n += (q.numel() + 3) // 4 * 4
        o.flat_p = torch.zeros(n)
        with torch.no_grad():
            for q, off in zip(o.params, o.offsets):
                o.flat_p[off:off + q.numel()].copy_(q.reshape(-1))
                q.data = o.flat_p[off:off + q.numel()].view(q.shape)
        return o

    with pytest.raises(ValueError, match="optimizers"):
        V.EMA(g, [])
    with pytest.raises(ValueError, match="vaegan_amd.Adam"):
        V.EMA(g, [torch.optim.Adam(g.parameters())])
    og, oh = fake_adam(g.parameters()), fake_adam(h.parameters())
    with pytest.raises(ValueError, match="optimizers"):
        V.EMA(g, [og] * 5)
    with pytest.raises(ValueError, match="not homed"):
        V.EMA(g, [oh])                                              # an optimizer that holds none of them
    with pytest.raises(ValueError, match="holds no parameter"):
        V.EMA(g, [og, oh])
    half = fake_adam(list(V.Generator(nz=16, ngf=16, img_size=16).parameters())[:2])
    with pytest.raises(ValueError, match="not homed"):
        V.EMA(g, [half])
    with torch.no_grad():                                           # homed once, then moved away from the flat buffer
        p0 = next(g.parameters())
        p0.data = p0.data.clone()
    with pytest.raises(ValueError, match="not homed"):
        V.EMA(g, [og])
    with pytest.raises(ValueError, match="constructor arguments"):
        lin = torch.nn.Linear(4, 4)
        V.EMA(lin, [fake_adam(lin.parameters())])
    # the networks record their constructor arguments where state_dict does not see them
    assert g._vg_ctor == dict(nz=16, ngf=16, nc=3, img_size=16, dtype="fp32") and "_vg_ctor" not in g.state_dict()
    e = V.Encoder([3, 64, 64], 10, dtype="bf16")
    assert e._vg_ctor == dict(img_size=[3, 64, 64], latent_dim=10, dtype="bf16")
    ema = V.EMA(h, [oh], decay=0.5, warmup=False)                   # construction itself needs no device
    sh = ema.module(h)
    assert type(sh) is V.Generator and not sh.training and not any(q.requires_grad for q in sh.parameters())
    assert list(sh.state_dict()) == list(h.state_dict())
    assert sh.main[1].running_mean is h.main[1].running_mean
    assert all(q.data_ptr() == ema.shadow_bufs[0].data_ptr() + 4 * off for q, off in zip(sh.parameters(), oh.offsets))
    with pytest.raises(ValueError, match="built over"):
        ema.module(g)
