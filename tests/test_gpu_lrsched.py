"""GPU: learning-rate schedules and decoupled weight decay (vg_step_prologue_sched, vg_adamw_apply in csrc/pack_adam.hip;
vaegan_amd.LRSchedule, vaegan_amd.AdamW, Adam(lr_schedule=)) -- the scheduled prologue against vg_step_prologue and the numpy
restatement of tests/_lrsched_ref.py, the AdamW launch against "multiply by state[3] in torch, then vg_adam_apply_clip" bit for
bit, and the options through the optimizers and the four trainers: what they leave alone, what they launch, twins stepped at
the host-evaluated rate, graph replay without re-capture, checkpoints, what loss_dict reports."""
import copy
import ctypes
import functools
import os
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _lrsched_ref as LR
import vaegan_amd as V
from _inputs import make_inputs

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, os.cpu_count() or 1))
DEV = "cuda"
PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
ops = import_module(PKG + ".ops")
L = import_module(PKG + "._lib")
F32 = np.float32
GUARD = 64
BASE = 2e-4
SENTINEL = -123.25


# ---- vg_step_prologue_sched -------------------------------------------------------------------------------------------
def c_rec(r):
    return None if r is None else L.LRSched(hold=r.hold, warmup=r.warmup, decay_start=r.decay_start, decay_len=r.decay_len,
                                            warmup_start=r.warmup_start, decay_param=r.decay_param,
                                            weight_decay=r.weight_decay, decay_kind=r.decay_kind, reserved=0)


def prologue(states, lrs, betas, recs=None, zero=None):
    """ONE vg_step_prologue_sched call (recs given, entries may be None) or vg_step_prologue call (recs None) over the rows of
    `states` ([k, 4] device tensor); checks that it is one launch."""
    k = states.shape[0]
    st = (ctypes.c_void_p * k)(*[states[i].data_ptr() for i in range(k)])
    lr = (ctypes.c_double * k)(*lrs)
    b1 = (ctypes.c_double * k)(*[b[0] for b in betas])
    b2 = (ctypes.c_double * k)(*[b[1] for b in betas])
    n0 = ops.launch_count()
    if recs is None:
        L.check(L.load().vg_step_prologue(None, st, lr, b1, b2, k, L.ptr(zero), 0 if zero is None else zero.numel(),
                                          L.stream_ptr()), "vg_step_prologue")
    else:
        keep = [c_rec(r) for r in recs]
        sc = (ctypes.c_void_p * k)(*[None if r is None else ctypes.addressof(r) for r in keep])
        L.check(L.load().vg_step_prologue_sched(None, st, lr, b1, b2, sc, k, L.ptr(zero), 0 if zero is None else zero.numel(),
                                                L.stream_ptr()), "vg_step_prologue_sched")
    assert ops.launch_count() - n0 == 1
    return states.cpu().numpy()


def states_at(ts):
    """[k, 4] device states whose step count is ts[i] - 1 and whose other slots hold a sentinel."""
    h = np.full((len(ts), 4), SENTINEL, dtype=F32)
    h[:, 0] = [t - 1 for t in ts]
    return torch.from_numpy(h).to(DEV)


PROLOGUE_SETS = [("warm_linear", "warm_cosine", "exp", "step"), ("step", "warm_const", "warm_cosine", "warm_linear")]
BETAS4 = [(0.5, 0.999), (0.9, 0.999), (0.9, 0.99), (0.5, 0.9)]
LRS4 = [2e-4, 1e-3, 3e-4, 0.05]


@pytest.mark.parametrize("names", PROLOGUE_SETS, ids=["a", "b"])
def test_scheduled_prologue_of_four_optimizers_against_the_plain_prologue_and_the_restatement(names):
    """One call over four optimizers with different kinds, betas and base rates, at every boundary step of any of the four.
      state[0], state[2]: vg_step_prologue's bits;
      warm-up / LINEAR / CONST (+ - * / only): state[3] equals the restatement bit for bit; state[1] = f32(lr_t / (1 - b1^t))
        within 2^-23 relative, the bound tests/test_gpu_optim.py holds the unscheduled state to (pow to an ulp);
      COSINE / EXP / STEP: state[1] and state[3] within one f32 ulp: the device's cos / pow are a few double ulps from numpy's,
        which can move the ONE narrowing to f32 across at most one rounding boundary."""
    recs = [LR.CASES[n] for n in names]
    steps = sorted(set().union(*[LR.boundary_steps(r) for r in recs]))
    zero = torch.full((8,), float("nan"), device=DEV)
    worst = 0
    for t in steps:
        got = prologue(states_at([t] * 4), LRS4, BETAS4, recs, zero)
        plain = prologue(states_at([t] * 4), LRS4, BETAS4)
        assert np.array_equal(got[:, [0, 2]].view(np.int32), plain[:, [0, 2]].view(np.int32)), t
        assert (got[:, 0] == t).all() and (plain[:, 3] == SENTINEL).all()
        for i, r in enumerate(recs):
            s1, s3 = LR.state1(LRS4[i], BETAS4[i][0], r, t), LR.state3(LRS4[i], r, t)
            if r.decay_kind in (LR.CONST, LR.LINEAR):
                assert got[i, 3].view(np.int32) == s3.view(np.int32), (names[i], t, got[i, 3], s3)
                np.testing.assert_allclose(got[i, 1], s1, rtol=2.0 ** -23, atol=0, err_msg=f"{names[i]} t={t}")
            else:
                d = (LR.ulp_distance(got[i, 1], s1), LR.ulp_distance(got[i, 3], s3))
                worst = max(worst, *d)
                assert max(d) <= 1, (names[i], t, got[i], s1, s3)
    assert torch.equal(zero, torch.zeros(8, device=DEV))
    print(f"{names}: {len(steps)} steps, worst ulp distance of the cos / pow kinds {worst}")


def test_null_entries_are_the_plain_prologue_and_leave_the_fourth_slot_alone():
    for t in (1, 2, 7, 40):
        got = prologue(states_at([t] * 3), LRS4[:3], BETAS4[:3], [None, None, None])
        plain = prologue(states_at([t] * 3), LRS4[:3], BETAS4[:3])
        assert np.array_equal(got.view(np.int32), plain.view(np.int32)) and (got[:, 3] == SENTINEL).all()
        # a NULL entry next to records: that lane alone is the plain one
        r = LR.CASES["warm_linear"]
        mixed = prologue(states_at([t] * 3), LRS4[:3], BETAS4[:3], [r, None, LR.Rec()])
        assert np.array_equal(mixed[1].view(np.int32), plain[1].view(np.int32))
        assert mixed[0, 3].view(np.int32) == LR.state3(LRS4[0], r, t).view(np.int32)
        # the constant record without decay: the plain lane's bits, and 1 in the fourth slot
        assert np.array_equal(mixed[2, :3].view(np.int32), plain[2, :3].view(np.int32)) and mixed[2, 3] == 1.0


# ---- vg_adamw_apply ---------------------------------------------------------------------------------------------------
CAP = 2048 * 256 * 4                              # elements the largest grid of one buffer covers in one pass
ADAMW_SIZES = [1, 3, 4, 5, 1027, CAP + 1027]


class Guarded:
    """A buffer between two 64-element sentinel guards (the buffer itself stays 16-byte aligned); tests/test_gpu_ema.py."""

    def __init__(self, values: torch.Tensor):
        n = values.numel()
        whole = torch.full((n + 2 * GUARD,), SENTINEL)
        whole[GUARD:GUARD + n] = values
        self.whole = whole.to(DEV)
        self.t = self.whole[GUARD:GUARD + n]

    def guards_intact(self) -> bool:
        return bool((self.whole[:GUARD] == SENTINEL).all()) and bool((self.whole[-GUARD:] == SENTINEL).all())


@functools.lru_cache(maxsize=None)
def draws(n, seed):
    """(p0, g, m0, v0) on the host, made once and never written: moments as after a few steps, so that every term is live."""
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=gen), torch.randn(n, generator=gen), 0.1 * torch.randn(n, generator=gen),
            0.01 * torch.rand(n, generator=gen))


def optimizer(n, seed, betas, eps, scale, state, decoupled, bad=False):
    """What ops.adam_apply_clip reads of an optimizer, every written buffer between guards."""
    p0, g, m0, v0 = draws(n, seed)
    if bad:                                       # non-finite parameters and gradients, in a vector lane and in the tail
        p0, g = p0.clone(), g.clone()
        for i, val in ((0, np.nan), (n // 2, np.inf), (n - 1, -np.inf)):
            p0[i] = val
            g[(i + 1) % n] = val
    bufs = [Guarded(p0), Guarded(m0), Guarded(v0)]
    o = SimpleNamespace(flat_p=bufs[0].t, flat_g=g.to(DEV), exp_avg=bufs[1].t, exp_avg_sq=bufs[2].t,
                        state_dev=torch.tensor(state, dtype=torch.float32, device=DEV), betas=betas, eps=eps, grad_scale=scale,
                        _DECOUPLED=decoupled, bufs=bufs)
    return o


def dev_coef(c):
    return None if c is None else torch.tensor([123.0, c], dtype=torch.float32, device=DEV)[1:]


def assert_same(a, b, what):
    for k in ("flat_p", "exp_avg", "exp_avg_sq"):
        x, y = getattr(a, k).cpu().numpy(), getattr(b, k).cpu().numpy()
        assert LR.same_bits(x, y), f"{what}: {k}"
    for o in (a, b):
        assert all(buf.guards_intact() for buf in o.bufs), f"{what}: a guard was written"


# [t, lr_t / (1 - b1^t), sqrt(1 - b2^t), 1 - lr_t * weight_decay] as a prologue leaves them; the decay factors are f32 values
# that are no power of two, the second far from 1 (lr 0.05, weight decay 2)
STATE_A = [3.0, 2.2857143e-4, 0.05474375, float(F32(1.0 - 2e-4 * 0.01))]
STATE_B = [3.0, 1.8450184e-2, 0.17277727, 0.9]


@pytest.mark.parametrize("n", ADAMW_SIZES)
def test_adamw_apply_of_one_buffer_equals_the_torch_product_then_the_clipped_launch(n):
    for coef in (None, 1.0, 0.37):
        for state, scale in ((STATE_A, 1.0), (STATE_B, 1.0 / 3.0)):
            a = optimizer(n, n % 1000 + 1, (0.5, 0.999), 1e-8, scale, state, True)
            ref = optimizer(n, n % 1000 + 1, (0.5, 0.999), 1e-8, scale, state, False)
            ref.flat_p.mul_(torch.tensor(state[3], dtype=torch.float32, device=DEV))       # one rounded f32 product
            g0 = a.flat_g.clone()
            n0 = ops.launch_count()
            ops.adam_apply_clip([a], [dev_coef(coef)])
            assert ops.launch_count() - n0 == 1
            ops.adam_apply_clip([ref], [dev_coef(coef)])
            assert_same(a, ref, f"n={n} coef={coef} decay={state[3]}")
            assert torch.equal(a.flat_g, g0), "the gradient is read only"
            assert torch.equal(a.state_dev.cpu(), torch.tensor(state)), "the state is read only"
        # weight_decay = 0 (state[3] = 1): vg_adam_apply_clip's bits
        one = STATE_A[:3] + [1.0]
        a = optimizer(n, n % 1000 + 2, (0.9, 0.999), 1e-8, 1.0, one, True)
        ref = optimizer(n, n % 1000 + 2, (0.9, 0.999), 1e-8, 1.0, one, False)
        ops.adam_apply_clip([a], [dev_coef(coef)])
        ops.adam_apply_clip([ref], [dev_coef(coef)])
        assert_same(a, ref, f"n={n} coef={coef} no decay")
        p0 = draws(n, n % 1000 + 2)[0]
        assert not torch.equal(a.flat_p.cpu(), p0)


@pytest.mark.parametrize("na,nb", [(5, 1027), (CAP + 1027, 3), (1, 1), (4, CAP + 1027)])
def test_adamw_apply_of_two_buffers_equals_the_torch_products_then_the_clipped_launch(na, nb):
    """The boundary between the two grids, each tail, the grid-stride loop of either; the buffers differ in betas, eps,
    grad_scale, coefficient and decay factor, so taking a setting from the wrong one shows."""
    for ca, cb in ((0.37, None), (None, 1.0), (1.0, 0.37)):
        mk = lambda dec: (optimizer(na, 5, (0.5, 0.999), 1e-8, 0.25, STATE_A, dec),          # noqa: E731
                          optimizer(nb, 6, (0.9, 0.99), 1e-6, 1.0 / 3.0, STATE_B, dec))
        a, b = mk(True)
        a2, b2 = mk(False)
        for o in (a2, b2):
            o.flat_p.mul_(o.state_dev[3])
        n0 = ops.launch_count()
        ops.adam_apply_clip([a, b], [dev_coef(ca), dev_coef(cb)])
        assert ops.launch_count() - n0 == 1
        ops.adam_apply_clip([a2, b2], [dev_coef(ca), dev_coef(cb)])
        assert_same(a, a2, f"first buffer, coefs {ca} {cb}")
        assert_same(b, b2, f"second buffer, coefs {ca} {cb}")


@pytest.mark.parametrize("n", [5, 1027])
def test_adamw_apply_propagates_non_finite_parameters_and_gradients(n):
    a = optimizer(n, 9, (0.5, 0.999), 1e-8, 1.0, STATE_B, True, bad=True)
    ref = optimizer(n, 9, (0.5, 0.999), 1e-8, 1.0, STATE_B, False, bad=True)
    ref.flat_p.mul_(ref.state_dev[3])
    ops.adam_apply_clip([a], [None])
    ops.adam_apply_clip([ref], [None])
    assert_same(a, ref, f"n={n} non-finite")
    p = a.flat_p.cpu().numpy()
    assert np.isnan(p[0]) and not np.isfinite(p[n // 2]) and not np.isfinite(p[n - 1]) and not np.isfinite(p[1])
    assert np.isfinite(p[2:n // 2]).all()


# ---- Adam / AdamW objects ---------------------------------------------------------------------------------------------
def small_net(cls=V.Adam, seed=1, **kw):
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Linear(37, 19), torch.nn.Linear(19, 3)).to(DEV)      # 37*19 + 19 + 57 + 3 parameters
    return net, cls(net.parameters(), lr=1e-2, **kw)


def fill_grads(opt, seed):
    g = torch.Generator().manual_seed(seed)
    for p in opt.params:
        p.grad.copy_(torch.randn(p.shape, generator=g))


SCHED = LR.CASES["warm_linear"].schedule(V)


def test_scheduled_step_equals_the_twin_stepped_at_the_host_rate_and_adamw_equals_torch():
    (_, a), (_, b) = small_net(lr_schedule=SCHED), small_net()
    assert a.scheduled and not b.scheduled and float(a.state_dev[3]) == 1.0 == float(b.state_dev[3])
    for k in range(12):
        for o in (a, b):
            fill_grads(o, 20 + k)
        b.lr = SCHED.lr(1e-2, k + 1)
        n0 = ops.launch_count()
        if k % 2:
            ops.step_prologue(None, [a])
            a.step(prepared=True)
        else:
            a.step()
        assert ops.launch_count() - n0 == 2
        b.step()
        for name in ("flat_p", "exp_avg", "exp_avg_sq"):
            assert torch.equal(getattr(a, name), getattr(b, name)), (k, name)
        assert torch.equal(a.state_dev[:3], b.state_dev[:3]) and float(a.state_dev[3]) == 1.0
        assert a.current_lr == b.lr == float(LR.lr_t(1e-2, LR.CASES["warm_linear"], k + 1)) and a.lr == 1e-2
    # AdamW against torch.optim.AdamW on the CPU at the scheduled rates, to the tolerances of tests/test_gpu_optim.py
    import test_gpu_optim as TO
    net, w = small_net(V.AdamW, weight_decay=0.1, lr_schedule=SCHED)
    ps = [torch.nn.Parameter(p.detach().cpu().clone()) for p in w.params]
    topt = torch.optim.AdamW(ps, lr=1e-2, weight_decay=0.1, foreach=False)
    for k in range(TO.STEPS):
        fill_grads(w, 40 + k)
        for q, p in zip(ps, w.params):
            q.grad = p.grad.detach().cpu().clone()
        topt.param_groups[0]["lr"] = SCHED.lr(1e-2, k + 1)
        topt.step()
        w.step()
    cat = lambda ts: torch.cat([t.detach().reshape(-1).cpu() for t in ts])                     # noqa: E731
    sd = w.state_dict()["state"]
    TO._compare((cat(w.params), cat([sd[i]["exp_avg"] for i in range(len(ps))]), cat([sd[i]["exp_avg_sq"] for i in range(len(ps))]),
                 float(w.state_dev[0])),
                (cat(ps), cat([topt.state[q]["exp_avg"] for q in ps]), cat([topt.state[q]["exp_avg_sq"] for q in ps]),
                 float(topt.state[ps[0]]["step"])), "AdamW object")
    assert float(w.state_dev[3]) == float(LR.state3(1e-2, LR.Rec(**{**LR.CASES["warm_linear"].__dict__, "weight_decay": 0.1}),
                                                    TO.STEPS))


def test_step_pair_with_one_adamw_decays_that_one_only_and_state_dict_round_trips():
    (_, a), (_, w) = small_net(seed=1), small_net(V.AdamW, seed=2, weight_decay=0.5)
    (_, a2), (_, w2) = small_net(seed=1), small_net(V.AdamW, seed=2, weight_decay=0.5)
    for o, s in ((a, 11), (w, 12), (a2, 11), (w2, 12)):
        fill_grads(o, s)
    ops.step_prologue(None, [a, w])
    n0 = ops.launch_count()
    a.step_pair(w)
    assert ops.launch_count() - n0 == 1
    a2.step(), w2.step()
    for x, y in ((a, a2), (w, w2)):
        for k in ("flat_p", "exp_avg", "exp_avg_sq", "state_dev"):
            assert torch.equal(getattr(x, k), getattr(y, k)), k
    assert float(a.state_dev[3]) == 1.0 and float(w.state_dev[3]) == float(F32(1.0 - 1e-2 * 0.5))
    sd = w.state_dict()
    assert set(sd) == {"state", "param_groups"} and set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    assert sd["param_groups"][0]["weight_decay"] == 0.5 and "lr_schedule" not in sd["param_groups"][0]
    assert set(a.state_dict()["param_groups"][0]) == {"lr", "betas", "eps", "weight_decay", "amsgrad", "params"}
    (_, s) = small_net(V.AdamW, seed=2, weight_decay=0.25, lr_schedule=SCHED)
    (_, r) = small_net(V.AdamW, seed=2)
    fill_grads(s, 30)
    s.step()
    r.load_state_dict(copy.deepcopy(s.state_dict()))
    r.flat_p.copy_(s.flat_p)
    assert r.lr_schedule == SCHED and r.weight_decay == 0.25 and r.steps == 1 and r.state_dev.tolist() == [1.0, 0.0, 0.0, 1.0]
    for o in (s, r):
        fill_grads(o, 31)
        o.step()
    for k in ("flat_p", "exp_avg", "exp_avg_sq", "state_dev"):
        assert torch.equal(getattr(s, k), getattr(r, k)), k
    with pytest.raises(NotImplementedError, match="AdamW"):
        a.load_state_dict(s.state_dict())
    plain = torch.optim.Adam([torch.nn.Parameter(p.detach().cpu().clone()) for p in a.params], lr=3e-3)
    a.load_state_dict(plain.state_dict())                               # a plain torch dict: accepted as before
    assert a.lr == 3e-3 and a.lr_schedule is None and a.weight_decay == 0.0
    # ... and into an AdamW: its decay becomes the dict's 0 (torch's own rule), its schedule, of which the dict says nothing, stays
    r.load_state_dict(torch.optim.Adam([torch.nn.Parameter(p.detach().cpu().clone()) for p in r.params], lr=3e-3).state_dict())
    assert r.lr == 3e-3 and r.weight_decay == 0.0 and r.lr_schedule == SCHED and r.steps == 0


# ---- through the trainers ---------------------------------------------------------------------------------------------
S, B, D_ITERS = 64, 4, 2
WARM = dict(warmup=4, warmup_start=0.25, decay="linear", decay_steps=6, final=0.1)
# the Discriminator's optimizer steps d_iters times per iteration: hold = d_iters moves its schedule once per iteration
SCHEDS = {"E": V.LRSchedule(**WARM), "G": V.LRSchedule(**WARM), "D": V.LRSchedule(**WARM, hold=D_ITERS)}
RECS = {"E": LR.CASES["warm_linear"], "G": LR.CASES["warm_linear"],
        "D": LR.Rec(**{**LR.CASES["warm_linear"].__dict__, "hold": D_ITERS})}


def build(opt=None, dtype="fp32", **kw):
    """opt(name, params) -> optimizer; None: V.Adam(params, lr=2e-4), the trainer built without the new arguments."""
    V.configure_seed(42)
    e = V.Encoder([3, S, S], 100, dtype=dtype)
    g = V.Generator(nz=100, img_size=S, dtype=dtype)
    d = V.Discriminator(img_size=S, dtype=dtype)
    g.apply(V.weights_init), d.apply(V.weights_init)
    e.to(DEV), g.to(DEV), d.to(DEV)
    opt = opt or (lambda name, params: V.Adam(params, lr=BASE))
    tr = V.VAEGANTrainer(e, g, d, *(opt(n, m.parameters()) for n, m in (("E", e), ("G", g), ("D", d))), d_iters=D_ITERS, **kw)
    tr.train()
    return e, g, d, tr


def scheduled(name, params):
    return V.Adam(params, lr=BASE, lr_schedule=SCHEDS[name])


def adamw(wd, sched=True):
    return lambda name, params: V.AdamW(params, lr=BASE, weight_decay=wd, lr_schedule=SCHEDS[name] if sched else None)


@functools.lru_cache(maxsize=None)
def batch(step):
    return tuple(t.to(DEV) for t in make_inputs(B, S, 7000 + S + step))


def full_state(e, g, d, tr):
    torch.cuda.synchronize()
    out = {}
    for n, m in (("E", e), ("G", g), ("D", d)):
        for k, v in m.state_dict().items():
            out[f"{n}.{k}"] = v.cpu().clone()
    for n, o in (("E", tr.opt_E), ("G", tr.opt_G), ("D", tr.opt_D)):
        for a in ("flat_p", "exp_avg", "exp_avg_sq"):
            out[f"opt_{n}.{a}"] = getattr(o, a).cpu().clone()
        out[f"opt_{n}.state"] = o.state_dev[:3].cpu().clone()        # slot 3 belongs to the decay: compared where it is set
        out[f"opt_{n}.steps"] = torch.tensor(o.steps)
    return out


def assert_same_state(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        x, y = a[k], b[k]
        if x.dtype == torch.float32:
            x, y = x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)
        assert torch.equal(x, y), k


def run(t, steps, graphed=False, first=0, before=None):
    """-> (losses per step, launches per step, state after the last); before(k): called ahead of step k."""
    e, g, d, tr = t
    losses, launches = [], []
    for k in range(first, first + steps):
        if before is not None:
            before(k)
        real, ez, er, ec = batch(k)
        n0 = ops.launch_count()
        out = (tr.train_step_graphed if graphed else tr.train_step)(real, 60, ez, er, ec)
        launches.append(ops.launch_count() - n0)
        losses.append(out.cpu().clone())
    return losses, launches, full_state(e, g, d, tr)


@functools.lru_cache(maxsize=None)
def scheduled_eager(steps=6):
    return run(build(scheduled), steps)


def test_off_is_the_trainer_without_the_new_arguments():
    a = run(build(), 2)
    t = build(lambda name, params: V.Adam(params, lr=BASE, lr_schedule=None))
    b = run(t, 2)
    for x, y in zip(a[0], b[0]):
        assert torch.equal(x, y)
    assert a[1] == b[1], "lr_schedule=None changed the number of kernel launches"
    assert_same_state(a[2], b[2])
    tr = t[3]
    assert sorted(tr.loss_dict(epoch=60)) == sorted(list(V.LOSS_NAMES) + ["total"])
    assert all(float(o.state_dev[3]) == 1.0 and o.current_lr == BASE for o in (tr.opt_E, tr.opt_G, tr.opt_D))
    # ... and a schedule or a decay launches nothing more
    assert scheduled_eager()[1][:2] == a[1]
    assert run(build(adamw(0.1)), 1)[1] == a[1][:1]


def test_scheduled_trainer_equals_the_twin_whose_rates_are_set_on_the_host():
    e, g, d, tw = t = build()

    def set_rates(k):
        tw.opt_E.lr, tw.opt_G.lr = SCHEDS["E"].lr(BASE, k + 1), SCHEDS["G"].lr(BASE, k + 1)
        tw.opt_D.lr = SCHEDS["D"].lr(BASE, D_ITERS * k + 1)
        assert tw.opt_D.lr == SCHEDS["D"].lr(BASE, D_ITERS * k + D_ITERS)

    twin = run(t, 5, before=set_rates)
    sch = scheduled_eager(5)
    for k in range(5):
        assert torch.equal(twin[0][k], sch[0][k]), k
    assert_same_state(twin[2], sch[2])
    assert twin[1] == sch[1]


def test_graphed_scheduled_steps_replay_one_capture_equal_eager_and_report_the_rates():
    t = build(scheduled)
    tr = t[3]
    first = run(t, 3, graphed=True)                                 # eager warm-up, capture + replay, one replay
    g3 = tr._graph
    assert g3 is not None
    rest = run(t, 3, graphed=True, first=3)
    assert tr._graph is g3, "the moving rate re-captured the iteration"
    ea = scheduled_eager()
    for k in range(6):
        assert torch.equal((first[0] + rest[0])[k], ea[0][k]), k
    assert_same_state(rest[2], ea[2])
    ld = tr.loss_dict(epoch=60)
    assert sorted(ld) == sorted(list(V.LOSS_NAMES) + ["total", "lr_E", "lr_G", "lr_D"])
    assert ld["lr_E"] == ld["lr_G"] == float(LR.lr_t(BASE, RECS["E"], 6)) and ld["lr_D"] == float(LR.lr_t(BASE, RECS["D"], 12))
    assert ld["lr_E"] != BASE and tr.opt_E.lr == BASE and tr.opt_E.param_groups[0]["lr"] == BASE
    # replacing the schedule: the old graph is not replayed
    key = g3.key
    tr.opt_G.set_schedule(V.LRSchedule(**{**WARM, "final": 0.5}))
    run(t, 1, graphed=True, first=6)
    assert tr._graph is None
    run(t, 1, graphed=True, first=7)
    assert tr._graph is not None and tr._graph.key != key


def test_adamw_trainer_graphed_equals_eager_also_with_clipping_and_differs_from_no_decay():
    ea = run(build(adamw(0.1)), 4)
    t = build(adamw(0.1))
    gr = run(t, 4, graphed=True)
    assert t[3]._graph is not None
    for k in range(4):
        assert torch.equal(ea[0][k], gr[0][k]), k
    assert_same_state(ea[2], gr[2])
    for n, o in (("E", t[3].opt_E), ("G", t[3].opt_G), ("D", t[3].opt_D)):
        want = LR.state3(BASE, LR.Rec(**{**RECS[n].__dict__, "weight_decay": 0.1}), o.steps)
        assert float(o.state_dev[3]) == float(want) < 1.0, n
    nodecay = run(build(adamw(0.0)), 4)
    assert not torch.equal(nodecay[2]["opt_G.flat_p"], ea[2]["opt_G.flat_p"])
    assert_same_state(nodecay[2], scheduled_eager(4)[2])            # weight_decay = 0: the scheduled Adam's bits
    ce = run(build(adamw(0.1), max_grad_norm=1e-2), 3)
    tc = build(adamw(0.1), max_grad_norm=1e-2)
    cg = run(tc, 3, graphed=True)
    for k in range(3):
        assert torch.equal(ce[0][k], cg[0][k]), k
    assert_same_state(ce[2], cg[2])
    assert (tc[3].grad_norms[:, 1] < 1.0).all() and not torch.equal(ce[2]["opt_E.flat_p"], ea[2]["opt_E.flat_p"])


def test_checkpoint_mid_warmup_resumes_bit_identically():
    whole = run(build(adamw(0.05)), 4)
    t = build(adamw(0.05))
    run(t, 2)
    sd = copy.deepcopy(t[3].state_dict())
    assert sd["opt_E"]["param_groups"][0]["lr_schedule"] == SCHEDS["E"].state_dict() and sd["opt_E"]["param_groups"][0]["lr"] == BASE
    r = build(lambda name, params: V.AdamW(params, lr=1.0, weight_decay=0.0))      # the file brings rate, schedule and decay
    r[3].load_state_dict(sd)
    assert r[3].opt_D.lr_schedule == SCHEDS["D"] and r[3].opt_D.weight_decay == 0.05 and r[3].opt_D.steps == 2 * D_ITERS
    resumed = run(r, 2, first=2)
    for k in range(2):
        assert torch.equal(whole[0][2 + k], resumed[0][k]), k
    assert_same_state(whole[2], resumed[2])


def test_graphed_function_with_a_scheduled_optimizer_captures_once():
    from test_gpu_parity import _reference_shaped_step
    res = []
    for use_graph in (False, True):
        V.configure_seed(42)
        nets = (V.Encoder([3, S, S], 100), V.Generator(nz=100, img_size=S), V.Discriminator(img_size=S))
        nets[1].apply(V.weights_init), nets[2].apply(V.weights_init)
        for m in nets:
            m.to(DEV), m.train()
        opts = tuple(V.AdamW(m.parameters(), lr=BASE, weight_decay=0.01, lr_schedule=SCHEDS[n]) for n, m in zip("EGD", nets))
        step = _reference_shaped_step(*nets, *opts, torch.nn.BCELoss(), torch.nn.MSELoss(reduction="mean"))
        if use_graph:
            step = V.graphed(step, modules=nets, optimizers=opts)
        losses = [step(*batch(i), epoch=60).clone() for i in range(5)]
        if use_graph:
            assert len(step._graphs) == 1 and sum(step._seen.values()) == 2
        torch.cuda.synchronize()
        res.append((torch.stack(losses).cpu(), [o.flat_p.cpu() for o in opts], [o.steps for o in opts]))
    assert torch.equal(res[0][0], res[1][0]) and res[0][2] == res[1][2] == [5, 5, 10]
    for a, b in zip(res[0][1], res[1][1]):
        assert torch.equal(a, b)


# ---- the sibling trainers ---------------------------------------------------------------------------------------------
def sib_inputs(step):
    g = torch.Generator().manual_seed(8100 + step)
    real = torch.rand(B, 3, S, S, generator=g) * 2 - 1
    eps_img = torch.randn(B, 3, S, S, generator=g)
    eps_z = torch.randn(B, 100, generator=g)
    noise = torch.randn(B, 100, 1, 1, generator=g)
    return [t.to(DEV) for t in (real, eps_img, eps_z, noise)]


def build_vae(opt, **kw):
    V.configure_seed(42)
    e, g = V.Encoder([3, S, S], 100).to(DEV), V.Generator(nz=100, img_size=S).to(DEV)
    o = opt(list(e.parameters()) + list(g.parameters()), lr=1e-3)
    tr = V.VAETrainer(e, g, o, **kw)
    tr.train()
    return tr, [o], lambda k, graphed=False: (tr.step_graphed if graphed else tr.train_step)(*sib_inputs(k)[:3], epoch=25)


def build_gan(cls, opt, **kw):
    V.configure_seed(42)
    g, d = V.Generator(nz=100, img_size=S), V.Discriminator(img_size=S)
    g.apply(V.weights_init), d.apply(V.weights_init)
    g.to(DEV), d.to(DEV)
    oG, oD = (opt(m.parameters(), lr=2e-4, betas=(0.5, 0.999)) for m in (g, d))
    tr = cls(g, d, oG, oD, **kw)
    tr.train()

    def step(k, graphed=False):
        real, _, _, noise = sib_inputs(k)
        f = tr.step_graphed if graphed else tr.train_step
        return f(real, noise.unsqueeze(0).clone(), noise) if cls is V.WGANTrainer else f(real, noise)
    return tr, [oG, oD], step


SIBLINGS = {"vae": (build_vae, ("EG",)), "dcgan": (lambda opt, **kw: build_gan(V.DCGANTrainer, opt, **kw), ("G", "D")),
            "wgan": (lambda opt, **kw: build_gan(V.WGANTrainer, opt, critic_iters=1, **kw), ("G", "D"))}
SIB_SCHED = V.LRSchedule(**WARM)


def sib_scheduled(p, **kw):
    return V.Adam(p, lr_schedule=SIB_SCHED, **kw)


def sib_adamw(wd):
    return lambda p, **kw: V.AdamW(p, weight_decay=wd, lr_schedule=SIB_SCHED, **kw)


def sib_run(name, opt, steps, graphed=False, before=None, built=None, first=0, **kw):
    """`steps` iterations of sibling trainer `name` from iteration `first`, on a trainer built here with optimizers opt(params,
    ...) and trainer keywords kw, or on `built` = the first three entries of an earlier result.
    -> (trainer, optimizers, step function, losses, launches, optimizer state); before(opts, k): called ahead of step k."""
    tr, opts, step = built if built is not None else SIBLINGS[name][0](opt, **kw)
    losses, launches = [], []
    for k in range(first, first + steps):
        if before is not None:
            before(opts, k)
        n0 = ops.launch_count()
        losses.append(step(k, graphed).cpu().clone())
        launches.append(ops.launch_count() - n0)
    torch.cuda.synchronize()
    state = [getattr(o, a)[:3 if a == "state_dev" else None].clone() for o in opts
             for a in ("flat_p", "exp_avg", "exp_avg_sq", "state_dev")]     # slot 3 belongs to the decay
    return tr, opts, step, losses, launches, state


def sib_same(a, b, steps=None):
    """Losses (of the first `steps` iterations) bit-equal and, for whole runs, the optimizers' buffers too."""
    return all(torch.equal(x, y) for x, y in zip(a[3][:steps], b[3][:steps])) and \
        (steps is not None or all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a[5], b[5])))


@pytest.mark.parametrize("name", list(SIBLINGS))
def test_sibling_trainer_schedule_off_twin_one_capture_and_recapture(name):
    nets = SIBLINGS[name][1]

    def set_rates(opts, k):
        for o in opts:
            o.lr = SIB_SCHED.lr(o.defaults["lr"], k + 1)

    # off means off
    plain = sib_run(name, V.Adam, 2)
    off = sib_run(name, lambda p, **kw: V.Adam(p, lr_schedule=None, **kw), 2)
    assert sib_same(plain, off) and plain[4] == off[4] and off[0].lr_dict() == {}
    # 5 eager steps under warm-up + linear decay against the twin whose rates are set on the host; the plain step's launches
    ea5 = sib_run(name, sib_scheduled, 5)
    assert ea5[4][:2] == plain[4], "a schedule changed the number of kernel launches"
    assert sib_same(sib_run(name, V.Adam, 5, before=set_rates), ea5)
    # 6 graphed steps: the graph after step 3 is the graph after step 6, the state is the eager run's
    gr = sib_run(name, sib_scheduled, 3, graphed=True)              # eager warm-up, capture + replay, one replay
    tr, opts, step = gr[:3]
    g3 = tr._gstate
    assert g3 is not None and sib_same(gr, ea5, steps=3)
    rest = sib_run(name, None, 3, graphed=True, built=gr[:3], first=3)
    assert tr._gstate is g3, "the moving rate re-captured the iteration"
    ea6 = sib_run(name, None, 1, built=ea5[:3], first=5)            # the eager run's sixth step
    assert all(torch.equal(x, y) for x, y in zip(gr[3] + rest[3], ea5[3] + ea6[3]))
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(rest[5], ea6[5]))
    base = opts[0].defaults["lr"]
    assert tr.lr_dict() == {f"lr_{n}": float(LR.lr_t(base, LR.CASES["warm_linear"], 6)) for n in nets}
    # another schedule: the old graph is not replayed, and the next capture has another key
    key = g3.key
    opts[0].set_schedule(V.LRSchedule(**{**WARM, "final": 0.5}))
    step(6, True)
    assert tr._gstate is None
    step(7, True)
    assert tr._gstate is not None and tr._gstate is not g3 and tr._gstate.key != key


@pytest.mark.parametrize("name", list(SIBLINGS))
def test_sibling_trainer_adamw_graphed_equals_eager_also_with_clipping(name):
    plain = sib_run(name, V.Adam, 1)
    we, wg = sib_run(name, sib_adamw(0.1), 3), sib_run(name, sib_adamw(0.1), 3, graphed=True)
    assert sib_same(we, wg) and wg[0]._gstate is not None and we[4][:1] == plain[4]
    # weight_decay = 0 is the scheduled Adam bit for bit, weight_decay > 0 is not
    sch = sib_run(name, sib_scheduled, 3)
    assert sib_same(sib_run(name, sib_adamw(0.0), 3), sch) and not sib_same(we, sch)
    # with max_grad_norm also set: runs, every network clipped, graphed equals eager bit for bit
    ce = sib_run(name, sib_adamw(0.1), 3, max_grad_norm=1e-4)
    cg = sib_run(name, sib_adamw(0.1), 3, graphed=True, max_grad_norm=1e-4)
    assert sib_same(ce, cg) and cg[0]._gstate is not None
    assert torch.equal(ce[0].grad_norms.view(torch.int32), cg[0].grad_norms.view(torch.int32))
    assert (cg[0].grad_norms[:, 1] < 1.0).all() and (cg[0].grad_norms[:, 1] > 0.0).all() and not sib_same(ce, we)
