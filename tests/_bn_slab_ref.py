"""float64 numpy restatement of the ORDER in which csrc/bn_act.hip adds statistics slab rows, with slabs on which that order
shows in the f32 results.  No torch, no GPU.  Shared by tests/test_bn_slab_order_cpu.py and tests/test_gpu_bn_slab_order.py.

tests/_bn_ref.py makes every sum exact, so that any order gives the same bits; it cannot tell whether a kernel kept its
order.  Here the f64 sums round, and a kernel that adds the same rows in another order gives other bits.

The two orders (slabs [nparts][2][C] f32, every add in f64):
  ff   ff_slice_stats / slice_sums of the one-launch forms: part lane pl (0..15) adds its rows pl, pl + 16, ... one after
       the other onto +0; the sixteen lane sums are then added onto +0 in lane order.
  fin  slab_sums of the finalize kernels: plane pl (0..127) adds its rows pl, pl + 128, ... one after the other onto +0; the
       eight planes of a wave are combined by a butterfly over the plane index (1, 2, 4: ((0+1)+(2+3))+((4+5)+(6+7)), the
       add is commutative, so every lane of the butterfly holds the same bits); the sixteen wave sums are added in wave order
       starting from wave 0's.
  row  every row onto +0 in row order: what no kernel does.  It is identical to ff up to 16 rows (one row per lane, lanes in
       order) and to fin up to 3 rows; beyond that it must give other bits (differs()), or the case proves nothing.

Coefficient arithmetic after the sums is tests/_bn_ref.py's, with one addition: shift = beta - mean * scale is ONE rounding
(the compiler contracts it into an fma in bn_finalize*_kernel and in both branches of bn_fin_act_fwd_kernel; on _bn_ref's
dyadic operands the two forms agree, on these they do not).  It is computed exactly in rationals here.

What keeps y and dx independent of how the compiler contracts the elementwise passes (the one-launch backward contracts some
of a thread's eight elements and not others): x is a signed power of two in the forward cases, so scale * x is exact; in the
backward cases the coefficients handed in are _bn_ref's dyadic table, gamma * invstd and dy are powers of two and
xhat = (x - mean) * invstd is 0 or a signed power of two, so a * dz and b * xhat are exact and a * dz - b * xhat is rounded
once either way.
"""
from fractions import Fraction

import numpy as np

import _bn_ref as R

f32, f64 = np.float32, np.float64
FF_PL, FIN_PL, WAVE_PLANES = 16, 128, 8


# ---- the orders ------------------------------------------------------------------------------------------------------------
def _lanes(slabs, nl):
    """[G][nparts][2][C] -> per-lane sequential f64 sums [G][nl][2][C] (rows l, l + nl, ... onto +0)."""
    s = np.asarray(slabs, dtype=f32).astype(f64)
    G, n, two, C = s.shape
    trips = -(-n // nl)
    pad = np.zeros((G, trips * nl, two, C), f64)          # x + 0.0 == x for every x a lane can hold (never -0: sums start at +0)
    pad[:, :n] = s
    pad = pad.reshape(G, trips, nl, two, C)
    acc = np.zeros((G, nl, two, C), f64)
    for t in range(trips):
        acc = acc + pad[:, t]
    return acc


def ff_sums(slabs):
    """-> f64 (s1, s2) [G][C] in the order of ff_slice_stats / slice_sums."""
    lanes = _lanes(slabs, FF_PL)
    s = np.zeros_like(lanes[:, 0])
    for k in range(FF_PL):
        s = s + lanes[:, k]
    return s[:, 0], s[:, 1]


def fin_sums(slabs):
    """-> f64 (s1, s2) [G][C] in the order of slab_sums."""
    lanes = _lanes(slabs, FIN_PL)
    G, _, two, C = lanes.shape
    w = lanes.reshape(G, FIN_PL // WAVE_PLANES, WAVE_PLANES, two, C)
    for o in (1, 2, 4):                                     # butterfly: plane j <- plane j + plane j ^ o
        w = w + w[:, :, np.arange(WAVE_PLANES) ^ o]
    w = w[:, :, 0]
    s = w[:, 0]
    for k in range(1, w.shape[1]):
        s = s + w[:, k]
    return s[:, 0], s[:, 1]


def row_sums(slabs):
    s = np.asarray(slabs, dtype=f32).astype(f64)
    acc = np.zeros_like(s[:, 0])
    for p in range(s.shape[1]):
        acc = acc + s[:, p]
    return acc[:, 0], acc[:, 1]


ORDER = {"ff": ff_sums, "fin": fin_sums}
SAME_AS_ROW_UP_TO = {"ff": 16, "fin": 3}


def differs(a, b):
    """Per group: does any channel of the f32 casts of the sums (s1, s2) differ in bits?  -> bool [G]."""
    d = np.zeros(a[0].shape[0], bool)
    for u, v in zip(a, b):
        d |= (u.astype(f32).view(np.uint32) != v.astype(f32).view(np.uint32)).any(1)
    return d


# ---- exact single rounding ---------------------------------------------------------------------------------------------------
def _to_f32(q):
    """Fraction -> the nearest f32, ties to even."""
    c = f32(float(q))                                         # within one ulp; settle it among the neighbours exactly
    cands = sorted({float(np.nextafter(c, f32(-np.inf))), float(c), float(np.nextafter(c, f32(np.inf)))})
    best = min(cands, key=lambda v: (abs(Fraction(v) - q), f32(v).view(np.uint32) & 1))
    return f32(best)


def fma_neg(a, b, c):
    """c - a * b in one rounding, elementwise on f32 arrays."""
    a, b, c = (np.asarray(v, dtype=f32) for v in np.broadcast_arrays(a, b, c))
    out = np.empty(a.shape, f32)
    for i in np.ndindex(a.shape):
        out[i] = _to_f32(Fraction(float(c[i])) - Fraction(float(a[i])) * Fraction(float(b[i])))
    return out


def finalize(s1, s2, count, gamma, beta, rmean, rvar, momentum, eps):
    """_bn_ref.finalize with the shift in one rounding."""
    co, rm, rv = R.finalize(s1, s2, count, gamma, beta, rmean, rvar, momentum, eps)
    bt = np.zeros(co.shape[2], f32) if beta is None else np.asarray(beta, dtype=f32)
    co[:, 3] = fma_neg(co[:, 0], co[:, 2], bt[None, :])
    return co, rm, rv


# ---- slabs on which the order shows ------------------------------------------------------------------------------------------
def _mag(rng, shape, lo, hi):
    return (np.exp2(rng.integers(lo, hi + 1, shape).astype(f64)) * rng.uniform(1.0, 2.0, shape)).astype(f32)


def order_slabs(seed, groups, nparts, C, small, big, positive=(False, False)):
    """[groups][nparts][2][C] f32.  Per (group, row kind, channel) a third of the rows hold pairs +v, -v (|v| in the binades
    `big`) dealt over random rows, the rest values in the binades `small` (random signs unless positive[kind]).  The pairs
    cancel in exact arithmetic; in f64 what is left of them depends on the order, and it is of the size of the small sum's
    last f32 bits or more.  small, big: per row kind (lo, hi) binary exponents, more than 40 apart."""
    rng = np.random.default_rng(seed)
    out = np.empty((groups, nparts, 2, C), f32)
    npair = nparts // 3
    for kind in range(2):
        v = _mag(rng, (groups, nparts, C), *small[kind])
        if not positive[kind]:
            v = v * rng.choice(np.array([-1, 1], f32), v.shape)
        if npair:
            b = _mag(rng, (groups, npair, C), *big[kind])
            v[:, 0:2 * npair:2] = b
            v[:, 1:2 * npair:2] = -b
        out[:, :, kind] = rng.permuted(v, axis=1)             # another permutation of the rows per (group, channel)
    return out


FWD_SMALL, FWD_BIG = ((-24, -20), (-8, -4)), ((20, 24), (38, 42))         # sum x: 48 binades; sum x*x (positive): 50
BWD_SMALL, BWD_BIG = ((-2, 2), (-2, 2)), ((46, 50), (46, 50))             # 52 binades


def fwd_case(seed, groups, nparts, C, momentum=0.5):
    """momentum 0.5 makes both products of the running update exact, so its result does not depend on whether the compiler
    contracts one of them into the sum (it does in bn_fin_act_fwd_kernel); the finalize kernels spell the update out
    uncontracted (running_update), as _bn_ref.finalize computes it, and take momentum 0.1."""
    rng = np.random.default_rng(seed + 1)
    return dict(slabs=order_slabs(seed, groups, nparts, C, FWD_SMALL, FWD_BIG, (False, True)),
                gamma=rng.normal(1.0, 0.3, C).astype(f32), beta=rng.normal(0.0, 0.5, C).astype(f32),
                rmean=(rng.normal(0.0, 1.0, C) * 2.0 ** -28).astype(f32), rvar=(rng.uniform(0.5, 2.0, C) * 2.0 ** -13).astype(f32),
                momentum=momentum, eps=1e-5)


def bwd_case(seed, groups, nparts, C):
    """gamma and invstd from _bn_ref's power-of-two tables (a = gamma * invstd exact); small initial dgamma / dbeta."""
    rng = np.random.default_rng(seed + 2)
    return dict(slabs=order_slabs(seed + 3, groups, nparts, C, BWD_SMALL, BWD_BIG),
                gamma=R._tab(R._GAMMA, C, 1, 0)[0], invstd=R._tab(R._IS, C, groups, 1),
                dgamma=rng.normal(0.0, 1.0, C).astype(f32), dbeta=rng.normal(0.0, 1.0, C).astype(f32))


def pow2_x(seed, rows, C):
    """Forward data: 0 and signed powers of two 2^-2 .. 2^3 (bf16), so that scale * x is exact."""
    rng = np.random.default_rng(seed + 4)
    x = np.exp2(rng.integers(-2, 4, (rows, C)).astype(f64)) * rng.choice([-1.0, 1.0], (rows, C))
    x[rng.random((rows, C)) < 0.05] = 0.0
    return x.astype(f32)


def bwd_data(seed, rpg, groups, C):
    """Backward data on _bn_ref.stream_coeffs(): x = mean + xhat / invstd with xhat in {0, +-1, +-2, +-4} (bf16: at most
    |mean| + 4 in steps of 1/2), dy a signed power of two 2^-8 .. 2^-5.  -> x, dy [groups * rpg][C], coeffs [groups][4][C]."""
    rng = np.random.default_rng(seed + 5)
    coeffs, _, _ = R.stream_coeffs(groups, C)
    xh = np.exp2(rng.integers(0, 3, (groups, rpg, C)).astype(f64)) * rng.choice([-1.0, 1.0], (groups, rpg, C))
    xh[rng.random(xh.shape) < 0.1] = 0.0
    x = coeffs[:, 0][:, None, :].astype(f64) + xh / coeffs[:, 1][:, None, :].astype(f64)
    dy = np.exp2(rng.integers(-8, -4, (groups, rpg, C)).astype(f64)) * rng.choice([-1.0, 1.0], (groups, rpg, C))
    x, dy = x.reshape(groups * rpg, C).astype(f32), dy.reshape(groups * rpg, C).astype(f32)
    assert (R.bf16_round(x) == x).all() and (R.bf16_round(dy) == dy).all()
    return x, dy, coeffs


# ---- case tables -------------------------------------------------------------------------------------------------------------
FUSED_C, FUSED_GROUPS, FUSED_NPARTS, FUSED_RPG = (64, 128), (1, 2, 3), (1, 15, 16, 17, 33, 199, 200), (130, 300)
FUSED_ACTS = ((R.ACT_RELU, 0.0), (R.ACT_LRELU, 0.25))
FUSED_CASES = [(C, g, n) for C in FUSED_C for g in FUSED_GROUPS for n in FUSED_NPARTS]
FIN_C, FIN_GROUPS = (8, 20, 64), (1, 2, 3)
FIN_NPARTS = (1, 127, 128, 129, 384, 385, 512, 513, 1024, 2049)
FIN_CASES = [(C, g, n) for C in FIN_C for g in FIN_GROUPS for n in FIN_NPARTS]
FIN_COUNT, FIN_MOMENTUM = 4096, 0.1


def seed_of(kind, C, groups, nparts):
    return {"ff": 10000, "fin": 50000}[kind] + 1000 * groups + 7 * nparts + C
