"""Adam with the constructor / zero_grad / step / state_dict surface of ``torch.optim.Adam`` as the
reference uses it (vaegan_code.py:42-44: ``optim.Adam(net.parameters(), lr=2e-4)``), executed as ONE
HIP kernel over a flat fp32 buffer (vg_adam_step; arithmetic of torch 2.10 ``_single_tensor_adam``,
SURVEY.md A12 / App. A.5).

At construction the parameters are re-homed into one contiguous buffer (``p.data`` becomes a view)
and ``p.grad`` becomes a view into a matching flat gradient buffer, so:
  * ``zero_grad()`` is one memset (gradients read as zeros instead of ``None`` -- the only observable
    difference from the reference, which nobody on the hot path observes);
  * autograd and the direct engine both accumulate in place into that buffer;
  * data-parallel training all-reduces ONE large buffer per network (ddp.py), sized for xGMI;
  * ``clip_grad_norm_`` (torch.nn.utils.clip_grad_norm_, norm_type=2, error_if_nonfinite=False) reduces that buffer on the
    device and leaves the coefficient there; the gradients in ``flat_g`` / ``p.grad`` are NOT rewritten -- the next
    ``step()`` multiplies each gradient by the coefficient where it reads it (the second observable difference from torch:
    after the call ``p.grad`` still holds the unclipped gradient).
  * a learning-rate schedule (``LRSchedule``, ``lr_schedule=``) is a closed-form function of the step count that lives on the
    device: the iteration's prologue launch evaluates it there (vg_step_prologue_sched), so a captured iteration replays a
    moving rate without being captured again.  ``AdamW`` adds torch.optim.AdamW's decoupled weight decay as one more
    multiply in the update kernel (vg_adamw_apply).  DESIGN.md section 4.4k.
Construct it AFTER ``.to(device)`` (as vaegan_code.py:29-44 does); moving the module afterwards
would detach the parameters from the flat buffer.
"""
import math
import operator
from typing import Iterable, Sequence, Union

import torch

from . import ops
from .engine import bump_weights_epoch


class LRSchedule:
    """A learning-rate schedule as a closed form of the optimizer's step count (include/vaegan_hip.h "Learning-rate
    schedules"): linear warm-up from ``warmup_start`` to 1 over ``warmup`` scheduler steps, times a decay that begins at
    scheduler step ``decay_start`` (None: at ``warmup``, torch's SequentialLR([warm-up, decay], milestones=[warmup])):

      "constant"  1
      "linear"    1 -> ``final`` over ``decay_steps``           torch LinearLR(end_factor=final, total_iters=decay_steps)
      "cosine"    1 -> ``final`` over ``decay_steps``           torch CosineAnnealingLR(T_max=decay_steps, eta_min=lr * final);
                                                                past the end the factor STAYS at final (torch's rises again)
      "exp"       ``gamma`` ** k                                torch ExponentialLR(gamma)
      "step"      ``gamma`` ** (k // ``decay_steps``)           torch StepLR(step_size=decay_steps, gamma)

    The scheduler moves once per ``hold`` optimizer steps (hold = steps per epoch: the epoch-stepped usage).  The optimizer
    evaluates the same formulas on the device, in double, from its device-resident step count; factor() / lr() evaluate them
    here in Python floats.  Immutable; ValueError for anything the C side would reject."""
    KINDS = ("constant", "linear", "cosine", "exp", "step")          # index = VG_LRS_*
    __slots__ = ("hold", "warmup", "warmup_start", "decay", "decay_start", "decay_steps", "final", "gamma")

    def __init__(self, warmup=0, warmup_start=0.0, decay="constant", decay_start=None, decay_steps=1, final=0.0, gamma=1.0,
                 hold=1):
        def integer(name, v, lo):
            try:                                # any integer type (numpy's included: len(loader) arithmetic), no bool, no float
                i = None if isinstance(v, bool) else operator.index(v)
            except TypeError:
                i = None
            if i is None or i < lo:
                raise ValueError(f"LRSchedule: {name} must be an integer >= {lo}, got {v!r}")
            return i

        def real(name, v, lo, hi, open_lo=False):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not (lo <= v <= hi) or (open_lo and v == lo):
                raise ValueError(f"LRSchedule: {name} must be a number in {'(' if open_lo else '['}{lo}, {hi}], got {v!r}")
            return float(v)

        if decay not in self.KINDS:
            raise ValueError(f"LRSchedule: decay must be one of {', '.join(self.KINDS)}, got {decay!r}")
        put = lambda name, value: object.__setattr__(self, name, value)       # noqa: E731
        put("decay", decay)
        put("hold", integer("hold", hold, 1))
        put("warmup", integer("warmup", warmup, 0))
        put("warmup_start", real("warmup_start", warmup_start, 0.0, 1.0))
        put("decay_start", self.warmup if decay_start is None else integer("decay_start", decay_start, 0))
        put("decay_steps", integer("decay_steps", decay_steps, 1))
        put("final", real("final", final, 0.0, 1.0))
        put("gamma", real("gamma", gamma, 0.0, 1.0, open_lo=True))

    def __setattr__(self, name, value=None):
        raise AttributeError("LRSchedule is immutable (its fields key captured graphs and its hash): build another one and "
                             "hand it to Adam.set_schedule()")

    __delattr__ = __setattr__

    def factor(self, step: int) -> float:
        """lr_t / lr of optimizer step number `step` (counted from 1: the count after that step's increment)."""
        e = (max(int(step), 1) - 1) // self.hold
        w = self.warmup_start + (1.0 - self.warmup_start) * (e / self.warmup) if e < self.warmup else 1.0
        k = max(e - self.decay_start, 0)
        u = min(k, self.decay_steps)
        if self.decay == "linear":
            d = 1.0 + (self.final - 1.0) * (u / self.decay_steps)
        elif self.decay == "cosine":
            d = self.final + (1.0 - self.final) * 0.5 * (1.0 + math.cos(math.pi * u / self.decay_steps))
        elif self.decay == "exp":
            d = math.pow(self.gamma, k)
        elif self.decay == "step":
            d = math.pow(self.gamma, k // self.decay_steps)
        else:
            d = 1.0
        return w * d

    def lr(self, base: float, step: int) -> float:
        return float(base) * self.factor(step)

    def key(self):
        """What a captured iteration freezes of the schedule: every field (not the object's identity)."""
        return (self.hold, self.warmup, self.warmup_start, self.decay, self.decay_start, self.decay_steps, self.final, self.gamma)

    def state_dict(self):
        return dict(warmup=self.warmup, warmup_start=self.warmup_start, decay=self.decay, decay_start=self.decay_start,
                    decay_steps=self.decay_steps, final=self.final, gamma=self.gamma, hold=self.hold)

    def __eq__(self, other):
        return isinstance(other, LRSchedule) and self.key() == other.key()

    def __hash__(self):
        return hash(self.key())

    def __reduce__(self):                       # copy / pickle rebuild it from its fields (nothing may be assigned)
        return (_schedule_from, (self.state_dict(),))

    def __repr__(self):
        return "LRSchedule(" + ", ".join(f"{k}={v!r}" for k, v in self.state_dict().items()) + ")"


def _schedule_from(fields):
    return LRSchedule(**fields)


def sched_record(schedule, weight_decay):
    """The vg_lr_sched record of (schedule, weight_decay); schedule None: the constant schedule (the decay alone)."""
    s = schedule if schedule is not None else LRSchedule()
    kind = LRSchedule.KINDS.index(s.decay)
    return ops.L.LRSched(hold=s.hold, warmup=s.warmup, decay_start=s.decay_start, decay_len=s.decay_steps,
                         warmup_start=s.warmup_start, decay_param=s.gamma if s.decay in ("exp", "step") else s.final,
                         weight_decay=float(weight_decay), decay_kind=kind, reserved=0)


class Adam:
    _DECOUPLED = False          # AdamW: weight_decay is the decoupled decay

    def __init__(self, params: Iterable[torch.Tensor], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0,
                 amsgrad=False, lr_schedule=None):
        if amsgrad or (weight_decay != 0 and not self._DECOUPLED):
            raise NotImplementedError("only the torch.optim.Adam defaults used by the reference are implemented "
                                      "(weight_decay=0, amsgrad=False); for decoupled weight decay use vaegan_amd.AdamW")
        weight_decay = check_weight_decay(weight_decay)
        if lr_schedule is not None and not isinstance(lr_schedule, LRSchedule):
            raise ValueError(f"lr_schedule must be a vaegan_amd.LRSchedule or None, got {lr_schedule!r}")
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")                  # torch.optim.Adam's own check and wording
        self.params = [p for p in params]
        if not self.params:
            raise ValueError("optimizer got an empty parameter list")
        dev = self.params[0].device
        for p in self.params:
            if not p.is_cuda or p.dtype != torch.float32:
                raise RuntimeError("vaegan_amd.Adam needs float32 parameters on the MI355X ('cuda'); "
                                   "construct it after .to(device) as vaegan_code.py:29-44 does")
            if p.device != dev:
                raise RuntimeError("all parameters of one optimizer must live on one device")
        self.defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False)
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        # lr stays the BASE rate; the rate of step t is lr_schedule.lr(lr, t), evaluated on the device from state_dev[0]
        self.weight_decay, self.lr_schedule = weight_decay, lr_schedule
        # Placement in the flat buffers.  Default: parameter order.  A parameter tagged `_vg_follows = other` (the
        # Encoder's fc_logvar after fc_mu, nets.py) is homed directly behind `other`, so that the pair forms one
        # contiguous [2N, ...] operand.  Indices in state_dict() stay those of self.params.
        ids = {id(p): i for i, p in enumerate(self.params)}
        followers = {}
        for i, p in enumerate(self.params):
            q = getattr(p, "_vg_follows", None)
            if q is not None and id(q) in ids and ids[id(q)] != i:
                followers.setdefault(ids[id(q)], []).append(i)
        placed, order = set(), []

        def place(i):
            if i in placed:
                return
            placed.add(i)
            order.append(i)
            for j in followers.get(i, ()):
                place(j)

        for i, p in enumerate(self.params):
            q = getattr(p, "_vg_follows", None)
            if q is not None and id(q) in ids and ids[id(q)] != i and ids[id(q)] not in placed:
                continue                                      # comes right after its leader
            place(i)
        for i in range(len(self.params)):
            place(i)
        self.offsets, n = [0] * len(self.params), 0
        for i in order:
            self.offsets[i] = n
            n += (self.params[i].numel() + 3) // 4 * 4         # keep every parameter 16-byte aligned
        self.numel = n
        self.flat_p = torch.zeros(n, dtype=torch.float32, device=dev)
        self.flat_g = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=dev)
        # [t, lr_t/(1-b1^t), sqrt(1-b2^t), 1 - lr_t * weight_decay]; the last is written only by a scheduled prologue and
        # reads 1 until then, so that a plain Adam can share vg_adamw_apply's launch with an AdamW (step_pair)
        self.state_dev = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float32, device=dev)
        with torch.no_grad():
            for p, o in zip(self.params, self.offsets):
                self.flat_p[o:o + p.numel()].copy_(p.detach().reshape(-1))
                p.data = self.flat_p[o:o + p.numel()].view(p.shape)
                p.grad = self.flat_g[o:o + p.numel()].view(p.shape)
                p._vg_fresh = True
                p._vg_homed = p.grad.data_ptr()            # address of this parameter's slot in the flat gradient buffer
        self.grad_scale = 1.0                                   # 1/world_size under data parallelism
        self.steps = 0
        # gradient-norm clipping (clip_grad_norm_): [norm, coefficient] of the last reduction and its f64 workspace, both
        # allocated on first use; armed: the next step() / step_pair() applies clip_dev[1] and disarms
        self.clip_dev = None
        self.clip_ws = None
        self._clip_armed = False
        bump_weights_epoch(self.params)

    # -- torch.optim.Optimizer surface ---------------------------------------------------------------
    def _group(self, params):
        grp = dict(params=params, lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=self.weight_decay, amsgrad=False)
        if self.lr_schedule is not None:
            grp["lr_schedule"] = self.lr_schedule.state_dict()
        return grp

    @property
    def param_groups(self):
        return [self._group(self.params)]

    @property
    def scheduled(self) -> bool:
        """The prologue of this optimizer is vg_step_prologue_sched's: it has a schedule, or it is an AdamW (whose
        state_dev[3] is then rewritten every iteration, whatever is assigned to weight_decay)."""
        return self.lr_schedule is not None or self._DECOUPLED

    def sched_record(self):
        """The vg_lr_sched record of this optimizer, None for a plain Adam without a schedule."""
        return sched_record(self.lr_schedule, self.weight_decay) if self.scheduled else None

    def capture_key(self):
        """What a captured iteration freezes of the learning rate: the base rate, the schedule's fields and the decay --
        not the rate of the step, which the device works out from its own step count."""
        return (self.lr, None if self.lr_schedule is None else self.lr_schedule.key(), self.weight_decay)

    def set_schedule(self, lr_schedule) -> None:
        """Replace (or with None remove) the schedule.  The step count is kept: the next step uses the new schedule's rate
        at that count.  A captured iteration is keyed on the schedule's fields and is captured again."""
        if lr_schedule is not None and not isinstance(lr_schedule, LRSchedule):
            raise ValueError(f"lr_schedule must be a vaegan_amd.LRSchedule or None, got {lr_schedule!r}")
        self.lr_schedule = lr_schedule

    @property
    def current_lr(self) -> float:
        """The learning rate of the last step taken (of the first one, before any), from the host's step count: no device
        read.  Without a schedule: lr."""
        return self.lr if self.lr_schedule is None else self.lr_schedule.lr(self.lr, max(self.steps, 1))

    def zero_grad(self, set_to_none: bool = True, memset: bool = True) -> None:
        """Gradients become zero (one memset).  memset=False only re-arms the 'overwrite on next write' flags --
        enough for the direct engine, which writes every gradient exactly once before accumulating."""
        if memset:
            ops.memset_zero(self.flat_g)
        for p in self.params:
            p._vg_fresh = True

    def _rehome_grads(self) -> None:
        for p, o in zip(self.params, self.offsets):
            g = p.grad
            if g is None or g.data_ptr() != self.flat_g.data_ptr() + 4 * o:
                # someone replaced .grad (e.g. zero_grad(set_to_none=True) from foreign code): re-home it
                with torch.no_grad():
                    view = self.flat_g[o:o + p.numel()].view(p.shape)
                    if g is None:
                        view.zero_()
                    else:
                        view.copy_(g)
                    p.grad = view

    def step(self, closure=None, prepared: bool = False):
        """prepared=True: this iteration's ops.step_prologue() has already advanced the step counter and the bias
        corrections of this optimizer on the device; only the update kernel is launched.
        Armed by clip_grad_norm_: the update multiplies every gradient by grad_scale * clip_dev[1], read from the device
        (vg_adam_apply_clip; unprepared: after a one-optimizer ops.step_prologue, the same two launches and double arithmetic
        as vg_adam_step), and disarms.  With a schedule or a decay the unprepared step takes the same two-launch form (the
        prologue is then vg_step_prologue_sched's); an AdamW's update is vg_adamw_apply."""
        if closure is not None:
            raise NotImplementedError("closure is not supported")
        self._rehome_grads()
        if self._clip_armed or self.scheduled:
            coef = self.clip_dev[1:] if self._clip_armed else None
            self._clip_armed = False
            if not prepared:
                ops.step_prologue(None, [self])
            ops.adam_apply_clip([self], [coef])
        else:
            ops.adam_step(self.flat_p, self.flat_g, self.exp_avg, self.exp_avg_sq, self.lr, self.betas[0],
                          self.betas[1], self.eps, self.grad_scale, self.state_dev, prepared=prepared)
        self.steps += 1
        bump_weights_epoch(self.params)

    def step_pair(self, other: "Adam") -> None:
        """self.step(prepared=True); other.step(prepared=True) as ONE launch (both optimizers prepared by this iteration's
        ops.step_prologue); results are bit-identical to the two launches.  With either optimizer armed by clip_grad_norm_
        the launch is vg_adam_apply_clip (an unarmed one of the pair steps unclipped) and both disarm.  With an AdamW in the
        pair it is vg_adamw_apply (a plain Adam's state_dev[3] reads 1)."""
        for o in (self, other):
            for p, off in zip(o.params, o.offsets):
                g = p.grad
                if g is None or g.data_ptr() != o.flat_g.data_ptr() + 4 * off:
                    raise RuntimeError("step_pair needs every .grad homed in the optimizer's flat gradient buffer")
        if self._clip_armed or other._clip_armed or self._DECOUPLED or other._DECOUPLED:
            ops.adam_apply_clip([self, other], [o.clip_dev[1:] if o._clip_armed else None for o in (self, other)])
            self._clip_armed = other._clip_armed = False
        else:
            ops.adam_apply2(self, other)
        for o in (self, other):
            o.steps += 1
            bump_weights_epoch(o.params)

    def clip_grad_norm_(self, max_norm: float) -> torch.Tensor:
        """torch.nn.utils.clip_grad_norm_(self.params, max_norm) with the coefficient left on the device: see
        clip_grad_norm_ below.  Returns the 0-dim device view of the norm (no sync)."""
        return clip_grad_norm_(self, max_norm)

    def state_dict(self):
        st = {}
        for i, (p, o) in enumerate(zip(self.params, self.offsets)):
            st[i] = dict(step=torch.tensor(float(self.steps)),
                         exp_avg=self.exp_avg[o:o + p.numel()].view(p.shape).clone(),
                         exp_avg_sq=self.exp_avg_sq[o:o + p.numel()].view(p.shape).clone())
        return dict(state=st, param_groups=[self._group(list(range(len(self.params))))])

    def load_state_dict(self, sd):
        """Accepts a torch.optim.Adam state_dict (same format as state_dict() returns).  "lr_schedule" in the group restores
        the schedule; without the key the optimizer's own schedule is kept (a plain torch dict says nothing about it).  The
        group's weight_decay, a key every torch dict has, is taken as torch takes it: an AdamW's decay becomes the dict's (0
        from a plain torch Adam dict), and it must be 0 for an Adam.  No schedule state exists beyond the step
        count, which is saved: the resumed run evaluates the same rates."""
        grp = sd["param_groups"][0]
        wd = check_weight_decay(grp.get("weight_decay", 0))
        if wd != 0 and not self._DECOUPLED:
            raise NotImplementedError("this state_dict carries weight_decay != 0: load it into a vaegan_amd.AdamW")
        self.lr, self.betas, self.eps = float(grp["lr"]), tuple(float(b) for b in grp["betas"]), float(grp["eps"])
        self.weight_decay = wd
        if grp.get("lr_schedule") is not None:
            self.lr_schedule = LRSchedule(**grp["lr_schedule"])
        steps = 0
        with torch.no_grad():
            for i, (p, o) in enumerate(zip(self.params, self.offsets)):
                s = sd["state"].get(i)
                if s is None:
                    continue
                self.exp_avg[o:o + p.numel()].copy_(s["exp_avg"].reshape(-1))
                self.exp_avg_sq[o:o + p.numel()].copy_(s["exp_avg_sq"].reshape(-1))
                steps = int(float(s["step"]))
            self.steps = steps
            self.state_dev.copy_(torch.tensor([float(steps), 0.0, 0.0, 1.0]))


class AdamW(Adam):
    """torch.optim.AdamW: Adam with DECOUPLED weight decay (Loshchilov & Hutter) -- every parameter is multiplied by
    1 - lr_t * weight_decay before the Adam update, inside the update kernel (vg_adamw_apply); lr_t is the scheduled rate."""
    _DECOUPLED = True

    def __init__(self, params: Iterable[torch.Tensor], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                 amsgrad=False, lr_schedule=None):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, lr_schedule)


def check_weight_decay(weight_decay) -> float:
    """A weight decay as the optimizers accept it: a finite number >= 0.  ValueError otherwise (torch's wording)."""
    if isinstance(weight_decay, bool) or not isinstance(weight_decay, (int, float)) or not 0.0 <= weight_decay < math.inf:
        raise ValueError(f"Invalid weight_decay value: {weight_decay!r}")
    return float(weight_decay)


def lr_report(named_opts) -> dict:
    """{"lr_<name>": current_lr} over {name: optimizer} when any of them has a schedule, {} otherwise (the trainers'
    loss_dict / lr_dict)."""
    if all(o.lr_schedule is None for o in named_opts.values()):
        return {}
    return {f"lr_{k}": o.current_lr for k, o in named_opts.items()}


def check_max_norm(max_norm) -> float:
    """A clipping threshold as clip_grad_norm_ and the trainers' max_grad_norm accept it: a real number >= 0, +inf (monitor
    only) included.  ValueError otherwise."""
    if isinstance(max_norm, bool) or not isinstance(max_norm, (int, float)):
        raise ValueError(f"max_norm must be a number >= 0 (inf: monitor only), got {max_norm!r}")
    m = float(max_norm)
    if math.isnan(m) or m < 0.0:
        raise ValueError(f"max_norm must be a number >= 0 (inf: monitor only), got {max_norm!r}")
    return m


def clip_grad_norm_(optimizers: Union[Adam, Sequence[Adam]], max_norm):
    """torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2, error_if_nonfinite=False) for one Adam or a list of up to
    4, each clipped to its OWN norm (no joint norm), in ONE vg_grad_norm_clip call (two launches, no host sync; capturable):
    for every optimizer  norm = |grad_scale| * ||flat_g||_2  (an f64 sum in a fixed order; with grad_scale = 1/world_size after
    an all-reduce SUM, the norm of the averaged gradient) and  coef = min(1, max_norm / (norm + 1e-6)), NaN propagating, are
    written to its clip_dev = [norm, coef] on the device.

    The gradients are NOT rewritten: the call ARMS each optimizer, and its next step() / step_pair() multiplies every
    gradient by grad_scale * coef where it reads it, then disarms.  Call it directly before optimizer.step(), where the
    reference-shaped loop would call torch's function.  max_norm: one number for all, or one per optimizer; inf only reports
    the norm (coef = 1 for a finite norm: the step's bits are the unclipped step's).
    Returns the 0-dim device view of the norm for one Adam, a list of them for a list."""
    single = isinstance(optimizers, Adam)
    opts = list(optimizers) if isinstance(optimizers, (list, tuple)) else [optimizers]
    if not 1 <= len(opts) <= ops.L.VG_GNORM_MAX or not all(isinstance(o, Adam) for o in opts):
        raise ValueError(f"clip_grad_norm_ takes one vaegan_amd.Adam or a list of 1..{ops.L.VG_GNORM_MAX}")
    if isinstance(max_norm, (list, tuple)):
        if len(max_norm) != len(opts):
            raise ValueError("clip_grad_norm_: one max_norm, or one per optimizer")
        norms = [check_max_norm(m) for m in max_norm]
    else:
        norms = [check_max_norm(max_norm)] * len(opts)
    for o in opts:
        o._rehome_grads()
        dev = o.flat_g.device
        if o.clip_dev is None:
            o.clip_dev = torch.zeros(2, dtype=torch.float32, device=dev)
        if o.clip_ws is None:
            o.clip_ws = torch.empty(ops.L.VG_GNORM_MAX * ops.L.VG_GNORM_PARTS, dtype=torch.float64, device=dev)
    ops.grad_norm_clip([o.flat_g for o in opts], [o.grad_scale for o in opts], norms, [o.clip_dev for o in opts],
                       opts[0].clip_ws)
    for o in opts:
        o._clip_armed = True
    views = [o.clip_dev[0] for o in opts]
    return views[0] if single else views
