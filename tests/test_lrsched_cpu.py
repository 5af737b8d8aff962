"""No GPU: the restatement the scheduled prologue and the AdamW kernel are tested against (tests/_lrsched_ref.py) is itself
checked -- the schedules against torch.optim.lr_scheduler in f64, the AdamW update against torch.optim.AdamW in f32 -- and so
are vaegan_amd.LRSchedule's host evaluation, the exported symbols, every host-side argument check of vg_step_prologue_sched /
vg_adamw_apply, and the validation of LRSchedule / AdamW."""
import ctypes
import math
import os
import re
import warnings
from importlib import import_module

import numpy as np
import pytest
import torch

import _lrsched_ref as LR
import vaegan_amd as V
from vaegan_amd import AdamW, LRSchedule  # noqa: F401  (this file is about the feature: without it nothing here is collected)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
F32, F64 = np.float32, np.float64
Rec = LR.Rec
BASE = 2e-4
EPS64 = 2.0 ** -53


# ---- the schedules against torch --------------------------------------------------------------------------------------
def _dummy():
    return torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=BASE)


def _closed(sched, e):
    sched.last_epoch = e
    return float(sched._get_closed_form_lr()[0])


def _stepped(make, n):
    """lr of scheduler steps 0 .. n - 1 of make(optimizer), stepping a CPU SGD dummy."""
    opt = _dummy()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sched = make(opt)
        out = []
        for _ in range(n):
            out.append(float(opt.param_groups[0]["lr"]))
            opt.step()
            sched.step()
    return out


def _host_equals_restatement(s, r, t):
    """LRSchedule's Python floats against the numpy restatement: the same roundings, so the same bits, for the kinds of
    + - * / alone; cos and pow come from two libraries (libm, numpy's own), each within an ulp: 4 * 2^-53 relative."""
    got, want = s.lr(BASE, t), float(LR.lr_t(BASE, r, t))
    if r.decay_kind in (LR.CONST, LR.LINEAR):
        assert got == want, (r, t)
    else:
        assert abs(got - want) <= 4 * EPS64 * want, (r, t, got, want)


def _check(r: Rec, torch_lr, last_e, bound_of):
    """The restatement and LRSchedule's host evaluation at every optimizer step t up to scheduler step last_e, hold in {1, 3}:
    against torch_lr(e) within the relative bound bound_of(e), and against each other."""
    worst = 0.0
    for hold in (1, 3):
        rr = Rec(**{**r.__dict__, "hold": hold})
        s = rr.schedule(V)
        for t in range(1, (last_e + 1) * hold + 1):
            e = (t - 1) // hold
            got, want = float(LR.lr_t(BASE, rr, t)), torch_lr(e)
            rel = abs(got - want) / want
            worst = max(worst, rel / bound_of(e))
            assert rel <= bound_of(e), (rr, t, e, got, want, rel)
            _host_equals_restatement(s, rr, t)
    print(f"{r}: worst relative error / bound {worst:.3f}")


def test_linear_warmup_and_linear_decay_equal_torch_linearlr_closed_form():
    """Both sides are closed forms of <= 6 rounded f64 operations on values of order 1 (no cancellation: every factor is
    >= the smaller end factor): 8 * 2^-53 relative."""
    for W, s0 in ((1, 0.5), (4, 0.25), (7, 1e-3)):
        sched = torch.optim.lr_scheduler.LinearLR(_dummy(), start_factor=s0, end_factor=1.0, total_iters=W)
        _check(Rec(warmup=W, warmup_start=s0, decay_kind=LR.CONST, decay_start=W), lambda e: _closed(sched, e), W + 3,
               lambda e: 8 * EPS64)
    for T, end in ((1, 0.5), (6, 0.1), (9, 0.0 + 1e-2)):
        sched = torch.optim.lr_scheduler.LinearLR(_dummy(), start_factor=1.0, end_factor=end, total_iters=T)
        _check(Rec(decay_kind=LR.LINEAR, decay_start=0, decay_len=T, decay_param=end), lambda e: _closed(sched, e), T + 3,
               lambda e: 8 * EPS64)


def test_exp_and_step_equal_torch_closed_forms():
    """lr * gamma ** k on both sides: one pow (libm, <= 1 ulp; numpy and Python call the same one) and one product."""
    for gamma in (0.9, 0.5, 1.0):
        sched = torch.optim.lr_scheduler.ExponentialLR(_dummy(), gamma=gamma)
        _check(Rec(decay_kind=LR.EXP, decay_start=0, decay_param=gamma), lambda e: _closed(sched, e), 12, lambda e: 4 * EPS64)
        for size in (1, 3):
            sched2 = torch.optim.lr_scheduler.StepLR(_dummy(), step_size=size, gamma=gamma)
            _check(Rec(decay_kind=LR.STEP, decay_start=0, decay_len=size, decay_param=gamma), lambda e: _closed(sched2, e),
                   12, lambda e: 4 * EPS64)


def test_cosine_equals_torch_cosineannealinglr_closed_form_up_to_the_end_and_stays_there():
    T, end = 6, 0.1
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(_dummy(), T_max=T, eta_min=BASE * end)
    # eta_min + (lr - eta_min) (1 + cos) / 2 against lr (end + (1 - end) 0.5 (1 + cos)): <= 8 operations a side, sums of
    # positive terms (no cancellation), cos to an ulp of a value <= 1: 16 * 2^-53
    r = Rec(decay_kind=LR.COSINE, decay_start=0, decay_len=T, decay_param=end)
    _check(r, lambda e: _closed(sched, e), T, lambda e: 16 * EPS64)
    assert float(LR.lr_t(BASE, r, T + 1)) == BASE * end               # e = T: cos(pi) = -1 exactly
    for t in range(T + 1, 4 * T):                                     # torch's is periodic past T_max; this one stays
        assert float(LR.lr_t(BASE, r, t)) == BASE * end == r.schedule(V).lr(BASE, t)        # cos(pi) = -1 in both libraries
    assert _closed(sched, 2 * T) == pytest.approx(BASE)


@pytest.mark.parametrize("kind", ["cosine", "linear"])
def test_warmup_then_decay_equals_torch_sequentiallr_stepped(kind):
    """SequentialLR([LinearLR warm-up, decay], milestones=[W]) has no closed form: a CPU SGD dummy is stepped.  torch chains
    lr_e from lr_{e-1}.  The bound is counted from its recursions: one chained step is <= 8 rounded f64 operations (LinearLR:
    a product, two sums, a quotient, a product; CosineAnnealingLR: two cos, two sums, a quotient, a difference, a product, a
    sum), and its cancellations amplify a rounding by at most 8 at these parameters (1 + cos(pi 5 / 6) = 0.134 is the
    smallest divisor, lr - eta_min >= 0.06 lr the smallest difference before the last step, where the factor is exactly 0):
    64 * 2^-53 per chained step, (e + 1) steps, against the closed form's own 16 * 2^-53."""
    W, s0, T, end = 4, 0.25, 6, 0.1
    L = torch.optim.lr_scheduler

    def make(opt):
        warm = L.LinearLR(opt, start_factor=s0, end_factor=1.0, total_iters=W)
        dec = L.CosineAnnealingLR(opt, T_max=T, eta_min=BASE * end) if kind == "cosine" else \
            L.LinearLR(opt, start_factor=1.0, end_factor=end, total_iters=T)
        return L.SequentialLR(opt, [warm, dec], milestones=[W])

    last = W + T if kind == "cosine" else W + T + 3                   # the cosine is compared up to its end (see above)
    lrs = _stepped(make, last + 1)
    assert lrs[0] == BASE * s0 and abs(lrs[W] - BASE) <= 1e-12 * BASE
    r = Rec(warmup=W, warmup_start=s0, decay_kind=LR.COSINE if kind == "cosine" else LR.LINEAR, decay_start=W, decay_len=T,
            decay_param=end)
    _check(r, lambda e: lrs[e], last, lambda e: (64 * (e + 1) + 16) * EPS64)
    assert LRSchedule(warmup=W, warmup_start=s0, decay=kind, decay_steps=T, final=end).key() == r.schedule(V).key()  # None = warmup


def test_boundaries_of_the_named_cases():
    for name, r in LR.CASES.items():
        ts = LR.boundary_steps(r)
        f = [float(LR.factor(r, t)) for t in ts]
        assert all(0.0 <= x <= 1.0 for x in f), (name, f)
        assert float(LR.factor(r, 1)) == (r.warmup_start if r.warmup > 0 else 1.0), name
        if r.decay_kind == LR.COSINE:
            assert float(LR.factor(r, ts[-1])) == r.decay_param, name
        if r.decay_kind == LR.LINEAR:                                  # the formula's own rounding: 0.09999999999999998 for 0.1
            assert float(LR.factor(r, ts[-1])) == 1.0 + (r.decay_param - 1.0), name
        for t in ts:
            e = (t - 1) // r.hold
            assert LR.factor(r, t) == LR.factor(r, e * r.hold + 1), (name, t)          # constant within a hold
            _host_equals_restatement(r.schedule(V), r, t)
        s1, s3 = LR.state1(BASE, 0.5, r, 3), LR.state3(BASE, r, 3)
        assert s1.dtype == F32 and s3.dtype == F32 and 0.0 < s3 <= 1.0
    assert LR.state1(BASE, 0.9, None, 7) == F32(BASE / (1.0 - 0.9 ** 7))                # a NULL entry: vg_step_prologue's
    assert LR.state3(BASE, Rec(weight_decay=0.0), 5) == 1.0


# ---- AdamW against torch ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("betas", [(0.5, 0.999), (0.9, 0.999)], ids=["b0.5", "b0.9"])
@pytest.mark.parametrize("case", ["warm_linear", "step"])
def test_restated_adamw_equals_torch_adamw(case, betas):
    """torch.optim.AdamW (single-tensor f32 form, CPU) with param_groups[0]["lr"] set to the restated lr_t before each step,
    against adamw_step fed state1 / state2 / state3: the tolerances tests/test_gpu_optim.py holds the Adam kernel to against
    torch.optim.Adam (its _compare, imported).  The one new operation is the f32 product p * state3, and state3 is the very
    scalar torch multiplies by -- asserted bit for bit at every step."""
    import test_gpu_optim as TO
    r, eps, n = LR.CASES[case], 1e-8, 1029
    gen = torch.Generator().manual_seed(11)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) for _ in range(TO.STEPS)]
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([p], lr=BASE, betas=betas, eps=eps, weight_decay=r.weight_decay, foreach=False)
    q, m, v = p0.numpy().copy(), np.zeros(n, F32), np.zeros(n, F32)
    for k, g in enumerate(grads):
        t = k + 1
        lr = float(LR.lr_t(BASE, r, t))
        opt.param_groups[0]["lr"] = lr
        assert F32(1.0 - lr * r.weight_decay).view(np.int32) == LR.state3(BASE, r, t).view(np.int32)
        assert F32(lr / (1.0 - betas[0] ** t)).view(np.int32) == LR.state1(BASE, betas[0], r, t).view(np.int32)
        p.grad = g.clone()
        opt.step()
        q, m, v = LR.adamw_step(q, g.numpy(), m, v, LR.state1(BASE, betas[0], r, t), LR.state2(betas[1], t),
                                LR.state3(BASE, r, t), betas, eps)
    st = opt.state[p]
    TO._compare((torch.from_numpy(q), torch.from_numpy(m), torch.from_numpy(v), float(TO.STEPS)),
                (p.detach(), st["exp_avg"], st["exp_avg_sq"], float(st["step"])), f"restated AdamW {case} {betas}")
    plain = torch.nn.Parameter(p0.clone())
    o2 = torch.optim.Adam([plain], lr=BASE, betas=betas, eps=eps, foreach=False)
    for g in grads:
        plain.grad = g.clone()
        o2.step()
    assert not torch.equal(plain.detach(), p.detach())                # the decay and the schedule are not inert here


# ---- LRSchedule / AdamW validation ------------------------------------------------------------------------------------
def test_lrschedule_validation_and_surface():
    ok = dict(warmup=3, warmup_start=0.1, decay="cosine", decay_steps=5, final=0.1, hold=2)
    s = LRSchedule(**ok)
    assert s.decay_start == 3 and LRSchedule(**ok, decay_start=0).decay_start == 0
    assert LRSchedule(**s.state_dict()) == s and LRSchedule(**s.state_dict()).key() == s.key()
    assert s.key() != LRSchedule(**{**ok, "final": 0.2}).key() and hash(s) == hash(LRSchedule(**ok))
    assert LRSchedule().factor(1) == 1.0 == LRSchedule().factor(10 ** 6) and LRSchedule().lr(3e-4, 5) == 3e-4
    assert LRSchedule(**{**ok, "hold": np.int64(2), "warmup": np.int32(3)}) == s and type(LRSchedule(hold=np.int64(7)).hold) is int
    for name, value in (("final", 0.5), ("hold", 3), ("other", 1)):  # immutable: the fields key captured graphs and the hash
        with pytest.raises(AttributeError):
            setattr(s, name, value)
    with pytest.raises(AttributeError):
        del s.hold
    assert s.final == 0.1 and s.hold == 2
    import copy
    import pickle
    assert copy.deepcopy(s) == s and pickle.loads(pickle.dumps(s)) == s
    for bad in (dict(hold=0), dict(hold=1.5), dict(hold=np.float64(2.0)), dict(hold=True), dict(warmup=-1), dict(warmup=2.0), dict(warmup_start=-0.1),
                dict(warmup_start=1.5), dict(warmup_start=math.nan), dict(decay="poly"), dict(decay=None), dict(decay_start=-1),
                dict(decay_steps=0), dict(final=-0.1), dict(final=1.1), dict(final=math.nan), dict(gamma=0.0),
                dict(gamma=1.5), dict(gamma=-0.5), dict(gamma=math.nan), dict(gamma="0.9")):
        with pytest.raises(ValueError):
            LRSchedule(**{**ok, **bad})


def test_adamw_and_adam_argument_validation_without_a_device():
    for wd in (-0.1, math.inf, math.nan, "0.1", True):
        with pytest.raises(ValueError, match="weight_decay"):
            V.AdamW([torch.nn.Parameter(torch.zeros(1))], weight_decay=wd)
    with pytest.raises(NotImplementedError, match="AdamW"):
        V.Adam([torch.nn.Parameter(torch.zeros(1))], weight_decay=0.1)
    with pytest.raises(NotImplementedError):
        V.AdamW([torch.nn.Parameter(torch.zeros(1))], amsgrad=True)
    for cls in (V.Adam, V.AdamW):
        with pytest.raises(ValueError, match="lr_schedule"):
            cls([torch.nn.Parameter(torch.zeros(1))], lr_schedule="cosine")
        with pytest.raises(RuntimeError, match="MI355X"):             # valid arguments get as far as the device check
            cls([torch.nn.Parameter(torch.zeros(1))], lr_schedule=LRSchedule(warmup=2))
    assert issubclass(V.AdamW, V.Adam)


def _shell(cls, **kw):
    """An optimizer without buffers: what state_dict() / param_groups / current_lr read besides them."""
    o = cls.__new__(cls)
    o.params, o.offsets, o.steps = [], [], 0
    o.lr, o.betas, o.eps, o.weight_decay, o.lr_schedule = 2e-4, (0.5, 0.999), 1e-8, 0.0, None
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_state_dict_keys_without_a_schedule_are_unchanged_and_the_schedule_rides_in_the_group():
    plain = _shell(V.Adam)
    sd = plain.state_dict()
    assert set(sd) == {"state", "param_groups"}
    assert set(sd["param_groups"][0]) == {"lr", "betas", "eps", "weight_decay", "amsgrad", "params"}
    assert sd["param_groups"][0]["weight_decay"] == 0 and set(plain.param_groups[0]) == set(sd["param_groups"][0])
    assert plain.current_lr == 2e-4 and not plain.scheduled and plain.sched_record() is None
    assert plain.capture_key() == (2e-4, None, 0.0)
    s = LRSchedule(warmup=4, warmup_start=0.25, decay="linear", decay_steps=6, final=0.1)
    o = _shell(V.AdamW, lr_schedule=s, weight_decay=0.01)
    grp = o.state_dict()["param_groups"][0]
    assert set(grp) == {"lr", "betas", "eps", "weight_decay", "amsgrad", "params", "lr_schedule"}
    assert grp["lr"] == 2e-4 and grp["weight_decay"] == 0.01 and LRSchedule(**grp["lr_schedule"]) == s
    assert o.scheduled and o.capture_key() == (2e-4, s.key(), 0.01)
    for steps in (0, 1, 3, 7, 30):
        o.steps = steps
        assert o.current_lr == float(LR.lr_t(2e-4, LR.CASES["warm_linear"], max(steps, 1)))
    rec = o.sched_record()
    want = LR.CASES["warm_linear"]
    assert (rec.hold, rec.warmup, rec.warmup_start, rec.decay_kind, rec.decay_start, rec.decay_len, rec.decay_param,
            rec.weight_decay) == (want.hold, want.warmup, want.warmup_start, want.decay_kind, want.decay_start, want.decay_len,
                                  want.decay_param, want.weight_decay)
    assert _shell(V.AdamW).scheduled and _shell(V.AdamW).sched_record().decay_kind == LR.CONST
    o.set_schedule(None)
    assert "lr_schedule" not in o.state_dict()["param_groups"][0] and o.current_lr == 2e-4
    with pytest.raises(ValueError):
        o.set_schedule(3)


# ---- C ABI on the host ------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_the_abi_version_moved():
    L = import_module(PKG + "._lib")
    lib = L.load()
    src = open(os.path.join(ROOT, "include", "vaegan_hip.h")).read()
    assert int(re.search(r"#define\s+VG_ABI_VERSION\s+(\d+)", src).group(1)) == L.ABI_VERSION >= 26
    assert lib.vg_abi_version() == L.ABI_VERSION
    for name in ("vg_step_prologue_sched", "vg_adamw_apply"):
        assert name in L.SIGNATURES and name in src and getattr(lib, name) is not None
    assert "Learning-rate schedules and decoupled weight decay" in src and "typedef struct vg_lr_sched" in src
    for i, kind in enumerate(("CONST", "LINEAR", "COSINE", "EXP", "STEP")):
        assert int(re.search(rf"#define\s+VG_LRS_{kind}\s+(\d+)", src).group(1)) == getattr(L, f"VG_LRS_{kind}") == i
        assert getattr(LR, kind) == i and LRSchedule.KINDS[i] == LR.KIND_NAMES[i]
    assert int(re.search(r"#define\s+VG_PROLOGUE_MAX\s+(\d+)", src).group(1)) == L.VG_PROLOGUE_MAX
    fields = re.search(r"typedef struct vg_lr_sched \{(.*?)\} vg_lr_sched;", src, flags=re.S).group(1)
    assert re.findall(r"\b(\w+);", fields) == [f[0] for f in L.LRSched._fields_]
    assert ctypes.sizeof(L.LRSched) == 64
    for name in ("LRSchedule", "AdamW"):
        assert name in V.__all__ and getattr(V, name) is getattr(import_module(PKG + ".optim"), name)


ST0, Z0, RNG0 = 1 << 20, 2 << 20, 3 << 20                               # fake device addresses
EINVAL, EALIGN = -1, -2


def _rec(L, **kw):
    f = dict(hold=1, warmup=2, decay_start=2, decay_len=4, warmup_start=0.5, decay_param=0.5, weight_decay=0.01,
             decay_kind=L.VG_LRS_LINEAR, reserved=0)
    f.update(kw)
    return L.LRSched(**f)


def _prologue(lib, recs, n=None, rng=RNG0, zero=Z0, nzero=4, null=(), lr=None, states=None):
    k = max(len(recs), 1)
    arrs = dict(states=(ctypes.c_void_p * k)(*(states if states is not None else [ST0 + 16 * i for i in range(len(recs))])),
                lr=(ctypes.c_double * k)(*(lr if lr is not None else [2e-4] * len(recs))),
                b1=(ctypes.c_double * k)(*[0.5] * len(recs)), b2=(ctypes.c_double * k)(*[0.999] * len(recs)),
                sched=(ctypes.c_void_p * k)(*[None if r is None else ctypes.addressof(r) for r in recs]))
    for name in null:
        arrs[name] = None
    return lib.vg_step_prologue_sched(rng, arrs["states"], arrs["lr"], arrs["b1"], arrs["b2"], arrs["sched"],
                                      len(recs) if n is None else n, zero, nzero, None)


def test_c_abi_rejects_bad_scheduled_prologue_arguments_on_host():
    """Every call here is rejected before a launch: nothing valid is ever passed whole (fake addresses, NULL stream).  Each
    bad field stands alone in an otherwise valid record, as the only record and behind a NULL entry and a valid one."""
    L = import_module(PKG + "._lib")
    lib = L.load()
    good = _rec(L)
    # what vg_step_prologue checks
    assert _prologue(lib, [good], n=-1) == EINVAL and _prologue(lib, [good] * 5) == EINVAL
    for name in ("states", "lr", "b1", "b2", "sched"):
        assert _prologue(lib, [good], null=(name,)) == EINVAL, name
    assert _prologue(lib, [], rng=None) == EINVAL                       # nothing to do at all
    assert _prologue(lib, [good], nzero=-1) == EINVAL and _prologue(lib, [good], nzero=65) == EINVAL
    assert _prologue(lib, [good], zero=None, nzero=4) == EINVAL
    assert _prologue(lib, [good], states=[None]) == EINVAL
    assert _prologue(lib, [good], lr=[-1e-3]) == EINVAL and _prologue(lib, [None], lr=[-1e-3]) == EINVAL
    # every field of the record, alone; a bad record in ANY position
    KIND = {k: getattr(L, f"VG_LRS_{k}") for k in ("CONST", "LINEAR", "COSINE", "EXP", "STEP")}
    bad = [dict(hold=0), dict(hold=-3), dict(warmup=-1), dict(warmup_start=-0.01), dict(warmup_start=1.01),
           dict(warmup_start=math.nan), dict(decay_kind=5), dict(decay_kind=-1), dict(decay_start=-1), dict(weight_decay=-1e-9),
           dict(weight_decay=math.inf), dict(weight_decay=math.nan)]
    for kind in ("LINEAR", "COSINE"):
        bad += [dict(decay_kind=KIND[kind], **f) for f in (dict(decay_len=0), dict(decay_len=-2), dict(decay_param=-0.1),
                                                            dict(decay_param=1.1), dict(decay_param=math.nan))]
    for kind in ("EXP", "STEP"):
        bad += [dict(decay_kind=KIND[kind], **f) for f in (dict(decay_param=0.0), dict(decay_param=-0.5), dict(decay_param=1.5),
                                                            dict(decay_param=math.nan))]
    bad += [dict(decay_kind=KIND["STEP"], decay_len=0)]
    for f in bad:
        r = _rec(L, **f)
        assert _prologue(lib, [r]) == EINVAL, f
        assert _prologue(lib, [None, good, r]) == EINVAL, f


def _adamw_call(lib, p, g, m, v, n, state, coef, count=None, null=()):
    k = len(p)
    arrs = dict(p=(ctypes.c_void_p * k)(*p), g=(ctypes.c_void_p * k)(*g), m=(ctypes.c_void_p * k)(*m), v=(ctypes.c_void_p * k)(*v),
                n=(ctypes.c_int64 * k)(*n), b1=(ctypes.c_double * k)(*[0.5] * k), b2=(ctypes.c_double * k)(*[0.999] * k),
                eps=(ctypes.c_double * k)(*[1e-8] * k), gs=(ctypes.c_float * k)(*[1.0] * k), state=(ctypes.c_void_p * k)(*state),
                coef=(ctypes.c_void_p * k)(*coef))
    for name in null:
        arrs[name] = None
    return lib.vg_adamw_apply(arrs["p"], arrs["g"], arrs["m"], arrs["v"], arrs["n"], arrs["b1"], arrs["b2"], arrs["eps"],
                              arrs["gs"], arrs["state"], arrs["coef"], k if count is None else count, None)


def test_c_abi_rejects_bad_adamw_apply_arguments_on_host():
    """vg_adam_apply_clip's checks (tests/test_gradclip_cpu.py), on the new entry point."""
    lib = import_module(PKG + "._lib").load()
    P, G_, M, V_, ST, C = (i << 20 for i in range(1, 7))
    ok = dict(p=[P + 4], g=[G_], m=[M], v=[V_], n=[1024], state=[ST], coef=[C])      # gets as far as EALIGN

    def call(**kw):
        a = dict(ok)
        extra = {k: kw.pop(k) for k in ("count", "null") if k in kw}
        a.update(kw)
        return _adamw_call(lib, **a, **extra)

    assert call() == EALIGN and call(coef=[None]) == EALIGN          # a NULL coefficient entry is allowed
    assert call(count=0) == EINVAL and call(count=3) == EINVAL and call(count=-1) == EINVAL
    three = dict(p=[P] * 3, g=[G_] * 3, m=[M] * 3, v=[V_] * 3, n=[8] * 3, state=[ST] * 3, coef=[C] * 3)
    assert _adamw_call(lib, **three) == EINVAL
    for name in ("p", "g", "m", "v", "n", "b1", "b2", "eps", "gs", "state", "coef"):
        assert call(null=(name,)) == EINVAL, name
    for name in ("p", "g", "m", "v", "state"):
        assert call(**{name: [None]}) == EINVAL, name
    assert call(n=[0]) == EINVAL and call(n=[-1]) == EINVAL
    for name, base in (("g", G_), ("m", M), ("v", V_)):
        assert call(p=[P], **{name: [base + 8]}) == EALIGN, name
    two = dict(p=[P, P + (1 << 16)], g=[G_, G_ + (1 << 16)], m=[M, M + (1 << 16)], v=[V_, V_ + (1 << 16) + 4], n=[8, 8],
               state=[ST, ST + 16], coef=[None, C])
    assert _adamw_call(lib, **two) == EALIGN
    two.update(n=[8, 0])
    assert _adamw_call(lib, **two) == EINVAL
    two.update(n=[8, 8], state=[ST, None])
    assert _adamw_call(lib, **two) == EINVAL
