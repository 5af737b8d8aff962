"""Test infrastructure for learning-rate schedules and decoupled weight decay (include/vaegan_hip.h "Learning-rate schedules
and decoupled weight decay"), CPU only:

  Rec                    the fields of one vg_lr_sched record;
  lr_t                   the scheduled rate of optimizer step t, the header's formulas in numpy f64 scalars (every operation
                         rounded on its own: numpy does not contract);
  state1 / state3        what vg_step_prologue_sched leaves in state[1] / state[3], each narrowed once to f32;
  adamw_step             one AdamW update of f32 arrays, the per-element code of csrc/pack_adam.hip in numpy f32: the decay as
                         ONE rounded product p * state3, then the Adam update;
  boundary_steps         optimizer steps around every boundary of a schedule;
  ulp_distance / bits    f32 comparisons.
"""
from dataclasses import dataclass

import numpy as np

F32 = np.float32
F64 = np.float64
CONST, LINEAR, COSINE, EXP, STEP = range(5)
KIND_NAMES = ("constant", "linear", "cosine", "exp", "step")


@dataclass(frozen=True)
class Rec:
    hold: int = 1
    warmup: int = 0
    warmup_start: float = 0.0
    decay_kind: int = CONST
    decay_start: int = 0
    decay_len: int = 1
    decay_param: float = 1.0
    weight_decay: float = 0.0

    def schedule(self, V):
        """The vaegan_amd.LRSchedule with these fields."""
        p = dict(gamma=self.decay_param) if self.decay_kind in (EXP, STEP) else dict(final=self.decay_param)
        if self.decay_kind == CONST:
            p = {}
        return V.LRSchedule(warmup=self.warmup, warmup_start=self.warmup_start, decay=KIND_NAMES[self.decay_kind],
                            decay_start=self.decay_start, decay_steps=self.decay_len, hold=self.hold, **p)


def factor(r: Rec, t: int) -> np.float64:
    e = (int(t) - 1) // r.hold
    one = F64(1.0)
    w = F64(r.warmup_start) + (one - F64(r.warmup_start)) * (F64(e) / F64(r.warmup)) if e < r.warmup else one
    k = max(e - r.decay_start, 0)
    u = min(k, r.decay_len)
    if r.decay_kind == LINEAR:
        d = one + (F64(r.decay_param) - one) * (F64(u) / F64(r.decay_len))
    elif r.decay_kind == COSINE:
        d = F64(r.decay_param) + (one - F64(r.decay_param)) * F64(0.5) * (one + np.cos(F64(np.pi) * F64(u) / F64(r.decay_len)))
    elif r.decay_kind == EXP:
        d = np.power(F64(r.decay_param), F64(k))
    elif r.decay_kind == STEP:
        d = np.power(F64(r.decay_param), F64(k // r.decay_len))
    else:
        d = one
    return w * d


def lr_t(lr: float, r, t: int) -> np.float64:
    """r None (a NULL entry): lr."""
    return F64(lr) if r is None else F64(lr) * factor(r, t)


def state1(lr, beta1, r, t) -> np.float32:
    return F32(lr_t(lr, r, t) / (F64(1.0) - np.power(F64(beta1), F64(t))))


def state2(beta2, t) -> np.float32:
    return F32(np.sqrt(F64(1.0) - np.power(F64(beta2), F64(t))))


def state3(lr, r: Rec, t) -> np.float32:
    return F32(F64(1.0) - lr_t(lr, r, t) * F64(r.weight_decay))


def adamw_step(p, g, m, v, s1, s2, s3, betas, eps, gscale=1.0):
    """(p, m, v) f32 arrays after one update: adam_decay + adam_update of csrc/pack_adam.hip, operation by operation in f32
    (s1, s2, s3: state[1..3] as f32; gscale: grad_scale * coefficient, already one f32).  Where the compiler contracts a
    product into the sum that follows (and ATen's CPU kernels use a fused multiply-add) the sum is formed in f64 and narrowed:
    one rounding but for the rare double rounding, far inside the tolerances this is compared under."""
    p, g, m, v = (np.asarray(a, dtype=F32) for a in (p, g, m, v))
    w1, b2, w2, eps = F32(1.0 - betas[0]), F32(betas[1]), F32(1.0 - betas[1]), F32(eps)

    def fma(a, b, c):                      # a * b + c rounded once: the product of two f32 is exact in f64
        return (a.astype(F64) * np.asarray(b, dtype=F32).astype(F64) + c.astype(F64)).astype(F32)

    with np.errstate(all="ignore"):
        p = p * F32(s3)                    # the decay: a rounded product of its own
        gr = g * F32(gscale)               # and so is the scaled gradient
        d = gr - m
        m = fma(d, w1, m) if w1 < F32(0.5) else fma(-d, F32(1.0) - w1, gr)
        v = fma(v, b2, w2 * (gr * gr))
        denom = np.sqrt(v) / F32(s2) + eps
        p = fma(m / denom, -F32(s1), p)
    return p, m, v


def boundary_steps(r: Rec):
    """Optimizer steps t whose scheduler step e = (t - 1) // hold is 0, warmup - 1, warmup, decay_start, decay_start +
    decay_len, and beyond: the first and the last t of each such e, plus a few steps in between."""
    es = {0, 1, r.warmup - 1, r.warmup, r.warmup + 1, r.decay_start - 1, r.decay_start, r.decay_start + 1,
          r.decay_start + r.decay_len // 2, r.decay_start + r.decay_len - 1, r.decay_start + r.decay_len,
          r.decay_start + r.decay_len + 1, r.decay_start + 3 * r.decay_len + 2}
    ts = set()
    for e in es:
        if e >= 0:
            ts.update((e * r.hold + 1, e * r.hold + r.hold))
    return sorted(ts)


def ulp_distance(a, b) -> int:
    """Distance of two finite f32 of one sign in units in the last place."""
    return abs(int(F32(a).view(np.int32)) - int(F32(b).view(np.int32)))


def bits(x) -> np.ndarray:
    return np.asarray(x, dtype=F32).reshape(-1).view(np.int32)


def same_bits(a, b) -> bool:
    """Equal f32 bit patterns, except that any NaN equals any NaN."""
    a, b = np.asarray(a, dtype=F32).reshape(-1), np.asarray(b, dtype=F32).reshape(-1)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and bool(np.array_equal(na, nb)) and bool(np.array_equal(a[~na].view(np.int32), b[~nb].view(np.int32)))


# the four schedules the prologue test steps in ONE call, one of each kind that exists besides CONST, and what the CPU tests
# compare with torch: warm-up + linear, warm-up + cosine, exponential after a delay, step with a hold
CASES = {
    "warm_linear": Rec(hold=1, warmup=4, warmup_start=0.25, decay_kind=LINEAR, decay_start=4, decay_len=6, decay_param=0.1,
                       weight_decay=0.01),
    "warm_cosine": Rec(hold=3, warmup=3, warmup_start=0.1, decay_kind=COSINE, decay_start=3, decay_len=6, decay_param=0.1,
                       weight_decay=0.05),
    "exp": Rec(hold=1, warmup=0, warmup_start=0.0, decay_kind=EXP, decay_start=2, decay_len=1, decay_param=0.9, weight_decay=0.0),
    "step": Rec(hold=3, warmup=2, warmup_start=0.5, decay_kind=STEP, decay_start=2, decay_len=3, decay_param=0.5,
                weight_decay=0.1),
    "warm_const": Rec(hold=1, warmup=5, warmup_start=0.0, decay_kind=CONST, decay_start=5, weight_decay=0.0),
}
