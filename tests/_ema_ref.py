"""Test infrastructure for the weight-averaging kernel (vg_ema_update, csrc/ema.hip), CPU only: the numpy restatement of
the contract in include/vaegan_hip.h ("Weight averaging") -- in f32 operation by operation, and in f64 -- and the input
generator of the GPU tests with the conditions it guarantees.

Contract, per buffer:  t = state[0] (the optimizer's step count, already incremented)
    d = (float)(warmup ? fmin(decay, (1.0 + t) / (10.0 + t)) : decay)      double, narrowed once
    w = 1.0f - d                                                           f32
    ema = ema + w * (p - ema)                                              three rounded f32 operations, no fma
"""
import numpy as np

F32 = np.float32
MAG_LO, MAG_HI = 2.0 ** -10, 2.0 ** 4
W_MIN = 1e-4


def decay_f64(decay: float, warmup: bool, t: float) -> float:
    """The decay of step t in double (Python floats are IEEE doubles; min has fmin's result for non-NaN arguments)."""
    t = float(t)
    return min(float(decay), (1.0 + t) / (10.0 + t)) if warmup else float(decay)


def decay_f32(decay: float, warmup: bool, t: float) -> np.float32:
    return F32(decay_f64(decay, warmup, t))


def weight_f32(decay: float, warmup: bool, t: float) -> np.float32:
    return F32(F32(1.0) - decay_f32(decay, warmup, t))


def step_f32(ema: np.ndarray, p: np.ndarray, decay: float, warmup: bool, t: float) -> np.ndarray:
    """One update, every operation rounded to f32 on its own (numpy evaluates each ufunc in the arrays' dtype)."""
    assert ema.dtype == F32 and p.dtype == F32
    w = weight_f32(decay, warmup, t)
    with np.errstate(invalid="ignore", over="ignore"):
        diff = p - ema
        prod = w * diff
        out = ema + prod
    assert diff.dtype == prod.dtype == out.dtype == F32
    return out


def step_f64(ema: np.ndarray, p: np.ndarray, decay: float, warmup: bool, t: float) -> np.ndarray:
    """The same formula with nothing narrowed: d, w and the three operations in f64."""
    w = 1.0 - decay_f64(decay, warmup, t)
    return ema.astype(np.float64) + w * (p.astype(np.float64) - ema.astype(np.float64))


def inputs(n: int, seed: int):
    """(ema, p) f32 [n]: signs random, magnitudes 2^U(-10, 4) clipped into [2^-10, 2^4], about one value in 16 an exact 0
    (either sign of zero in p).  With a weight w >= 1e-4 (or w == 0) no intermediate of an update is subnormal: a nonzero
    difference of two such values is at least 2^-10 * 2^-23 = 2^-33 in magnitude, its product with w at least 2^-47, and a
    nonzero sum of two numbers that are multiples of 2^-70 and of normal magnitude is normal (check_conditions)."""
    rng = np.random.default_rng(seed)

    def one():
        mag = np.clip(np.exp2(rng.uniform(-10.0, 4.0, n)), MAG_LO, MAG_HI).astype(F32)
        mag = np.clip(mag, F32(MAG_LO), F32(MAG_HI))
        v = mag * rng.choice(np.array([-1.0, 1.0], dtype=F32), n)
        v[rng.random(n) < 1.0 / 16] = 0.0
        return v.astype(F32)

    ema, p = one(), one()
    p[(p == 0) & (rng.random(n) < 0.5)] = F32(-0.0)
    return ema, p


def check_conditions(ema: np.ndarray, p: np.ndarray, w: np.float32) -> None:
    """What the bitwise GPU comparisons rely on (flush-to-zero or not, the results are the same): magnitudes in range, the
    weight not tiny, and no subnormal intermediate."""
    tiny = np.finfo(F32).tiny
    for v in (ema, p):
        nz = np.abs(v[v != 0])
        assert v.dtype == F32 and (nz.size == 0 or (nz.min() >= F32(MAG_LO) and nz.max() <= F32(MAG_HI)))
    assert w == 0 or w >= F32(W_MIN)
    diff = p - ema
    prod = w * diff
    out = ema + prod
    for v in (diff, prod, out):
        nz = np.abs(v[v != 0])
        assert nz.size == 0 or nz.min() >= tiny


def same_bits(got: np.ndarray, want: np.ndarray) -> bool:
    """Bitwise equality on int32 views; where `want` is NaN, `got` must be NaN (payloads are the hardware's)."""
    assert got.dtype == F32 and want.dtype == F32 and got.shape == want.shape
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False
    return np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan])
