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
Construct it AFTER ``.to(device)`` (as vaegan_code.py:29-44 does); moving the module afterwards
would detach the parameters from the flat buffer.
"""
import math
from typing import Iterable, Sequence, Union

import torch

from . import ops
from .engine import bump_weights_epoch


class Adam:
    def __init__(self, params: Iterable[torch.Tensor], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0,
                 amsgrad=False):
        if weight_decay != 0 or amsgrad:
            raise NotImplementedError("only the torch.optim.Adam defaults used by the reference are implemented "
                                      "(weight_decay=0, amsgrad=False)")
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
        self.defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=0, amsgrad=False)
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
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
        self.state_dev = torch.zeros(4, dtype=torch.float32, device=dev)   # [t, lr/(1-b1^t), sqrt(1-b2^t), -]
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
    @property
    def param_groups(self):
        return [dict(params=self.params, lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=0, amsgrad=False)]

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
        as vg_adam_step), and disarms."""
        if closure is not None:
            raise NotImplementedError("closure is not supported")
        self._rehome_grads()
        if self._clip_armed:
            self._clip_armed = False
            if not prepared:
                ops.step_prologue(None, [self])
            ops.adam_apply_clip([self], [self.clip_dev[1:]])
        else:
            ops.adam_step(self.flat_p, self.flat_g, self.exp_avg, self.exp_avg_sq, self.lr, self.betas[0],
                          self.betas[1], self.eps, self.grad_scale, self.state_dev, prepared=prepared)
        self.steps += 1
        bump_weights_epoch(self.params)

    def step_pair(self, other: "Adam") -> None:
        """self.step(prepared=True); other.step(prepared=True) as ONE launch (both optimizers prepared by this iteration's
        ops.step_prologue); results are bit-identical to the two launches.  With either optimizer armed by clip_grad_norm_
        the launch is vg_adam_apply_clip (an unarmed one of the pair steps unclipped) and both disarm."""
        for o in (self, other):
            for p, off in zip(o.params, o.offsets):
                g = p.grad
                if g is None or g.data_ptr() != o.flat_g.data_ptr() + 4 * off:
                    raise RuntimeError("step_pair needs every .grad homed in the optimizer's flat gradient buffer")
        if self._clip_armed or other._clip_armed:
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
        grp = dict(lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=0, amsgrad=False,
                   params=list(range(len(self.params))))
        return dict(state=st, param_groups=[grp])

    def load_state_dict(self, sd):
        """Accepts a torch.optim.Adam state_dict (same format as state_dict() returns)."""
        grp = sd["param_groups"][0]
        self.lr, self.betas, self.eps = float(grp["lr"]), tuple(float(b) for b in grp["betas"]), float(grp["eps"])
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
            self.state_dev.zero_()
            self.state_dev[0] = float(steps)


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
