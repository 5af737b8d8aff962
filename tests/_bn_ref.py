"""numpy restatement of every stage of csrc/bn_act.hip (train / eval BatchNorm + ReLU / LeakyReLU on [rows][C] tensors of
`groups` equal row blocks), the integer operands on which every intermediate of those stages is exactly representable, and
the case tables of tests/test_bn_cpu.py and tests/test_gpu_bn.py.  No torch (the e4m3 twin alone borrows torch's cast), no GPU.

The arithmetic types are the kernels': the column reduce forms its terms and sums in f32, the slab sums and both finalizes
work in f64 and cast their results to f32 where the kernels do, the elementwise passes work in f32 and round once to the
storage type.  Every function takes `ft`: np.float32 restates the kernels, np.float64 is the same formulas without the f32
roundings (the reference of the float-valued finalize test, and what test_bn_cpu.py holds against torch autograd).

Layouts: x, dy [groups * rows_per_group][C]; coeffs [groups][4][C] = mean, invstd, scale, shift; coef [groups][3][C] =
a, b, c of dx = a * dz - b * xhat - c; slabs [groups][nparts][2][C].

Why integers.  A float reference cannot say which of two roundings is right: the separate kernels spell their contractions
out (__builtin_fmaf), the fused ones leave them to the compiler.  When every product and every sum is exact, a contracted and
an uncontracted evaluation, and every summation order, give the same bits -- so there is ONE right answer, this file computes
it, and the GPU tests compare with torch.equal.  sum_is_exact(), same_in_both() and fits_bf16() measure the conditions that make that true; test_bn_cpu.py
asserts them for every case.

The one intermediate that cannot be made exact is the unbiased variance var * (count / (count - 1)) of the running-variance
update.  finalize() performs the same two f64 operations in the same order as the kernels and the same cast to f32; what
follows, rv' = (1 - m) * rv + m * u, is kept to ONE rounding by the inputs: either rv == 0 (the sum is the product m * u,
rounded once whether or not it is contracted into an fma) or m in {0.5, 1} ((1 - m) * rv and m * u are then exact, and the
sum is rounded once either way).  From the second group on rv != 0, so grouped cases use m in {0.5, 1}.
"""
import numpy as np

F32, BF16 = 0, 1
ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2
f32, f64 = np.float32, np.float64


# ---- storage types -------------------------------------------------------------------------------------------------------
def bf16_round(a):
    """f32 -> the nearest bf16 (ties to even), returned as f32.  Finite values only."""
    a = np.ascontiguousarray(a, dtype=f32)
    assert np.isfinite(a).all()
    u = a.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return (r & 0xFFFFFFFF).astype(np.uint32).view(f32).reshape(a.shape)


def store(a, dtype, ft=f32):
    """What a kernel writes for the f32 value `a`: the value as stored (f32, or bf16-rounded), held in f32."""
    if ft is f64:
        return np.asarray(a, dtype=f64)
    return bf16_round(a) if dtype == BF16 else np.asarray(a, dtype=f32)


def e4m3_twin(y):
    """The e4m3 twin of a STORED bf16 activation: torch's float8_e4m3fn cast on the CPU (round to nearest even), as bytes."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(y, dtype=f32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


# ---- the restatement -----------------------------------------------------------------------------------------------------
def _fma(a, b, c, ft):
    """One rounding of a * b + c: the product of two f32 is exact in f64."""
    if ft is f64:
        return a * b + c
    return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)


def _grouped(t, groups, ft):
    t = np.asarray(t).astype(ft)
    assert t.shape[0] % groups == 0
    return t.reshape(groups, t.shape[0] // groups, t.shape[1])


def _per_group(v, ft):
    """[groups][C] coefficient -> broadcastable over the rows of each group."""
    return np.asarray(v).astype(ft)[:, None, :]


def act_fwd(z, act, slope):
    if act == ACT_RELU:
        return np.where(z > 0, z, z.dtype.type(0))
    if act == ACT_LRELU:
        return np.where(z > 0, z, z * z.dtype.type(slope))
    return z


def act_bwd(z, g, act, slope, zero_positive=False):
    """dy * act'(z); at z == 0 the derivative is the negative branch (zero_positive: the wrong choice, for the blind-spot
    check of test_bn_cpu.py)."""
    pos = (z >= 0) if zero_positive else (z > 0)
    if act == ACT_RELU:
        return np.where(pos, g, g.dtype.type(0))
    if act == ACT_LRELU:
        return np.where(pos, g, g * g.dtype.type(slope))
    return g


def col_stats(x, groups=1, ft=f32):
    """-> (sum x, sum x*x) [groups][C]: terms in ft, summed exactly (f64) and cast to ft -- the f32 sum of any order where
    sum_is_exact() holds."""
    xs = _grouped(x, groups, ft)
    return (xs.astype(f64).sum(1) + 0.0).astype(ft), ((xs * xs).astype(f64).sum(1) + 0.0).astype(ft)     # + 0.0: a sum starts at +0


def bwd_terms(x, dy, coeffs, act, slope, groups=1, ft=f32, zero_positive=False):
    """-> dz, dz * xhat [groups][rows_per_group][C] with dz = act'(sc * x + sh) * dy, xhat = (x - mu) * is."""
    xs, gs = _grouped(x, groups, ft), _grouped(dy, groups, ft)
    co = np.asarray(coeffs).astype(ft)
    mu, is_, sc, sh = (_per_group(co[:, k], ft) for k in range(4))
    dz = act_bwd(sc * xs + sh, gs, act, slope, zero_positive)
    return dz, dz * ((xs - mu) * is_)


def bwd_sums(x, dy, coeffs, act, slope, groups=1, ft=f32, zero_positive=False):
    """-> (sum dz, sum dz*xhat) [groups][C]."""
    dz, dzx = bwd_terms(x, dy, coeffs, act, slope, groups, ft, zero_positive)
    return (dz.astype(f64).sum(1) + 0.0).astype(ft), (dzx.astype(f64).sum(1) + 0.0).astype(ft)


def slab_sums(slabs):
    """[groups][nparts][2][C] f32 -> f64 (s1, s2) [groups][C] (bn_act.hip slab_sums: double accumulation)."""
    s = np.asarray(slabs, dtype=f32).astype(f64).sum(1) + 0.0
    return s[:, 0], s[:, 1]


def finalize(s1, s2, count, gamma, beta, rmean, rvar, momentum, eps, ft=f32):
    """bn_finalize_kernel / bn_finalize_grouped_kernel / bn_finalize_sums_kernel / the publisher of bn_fin_act_fwd_kernel:
    f64 sums [groups][C] -> coeffs [groups][4][C] and the running statistics updated group after group (None: none)."""
    s1, s2 = np.asarray(s1, dtype=f64), np.asarray(s2, dtype=f64)
    G, C = s1.shape
    count = f64(count)
    eps_d, m = f64(f32(eps)), ft(f32(momentum))
    gm = np.ones(C, ft) if gamma is None else np.asarray(gamma).astype(ft)
    bt = np.zeros(C, ft) if beta is None else np.asarray(beta).astype(ft)
    rm = None if rmean is None else np.asarray(rmean).astype(ft)
    rv = None if rvar is None else np.asarray(rvar).astype(ft)
    co = np.empty((G, 4, C), ft)
    for g in range(G):
        mu = s1[g] / count
        var = np.maximum(s2[g] / count - mu * mu, 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):             # var + eps == 0 gives inf, as in the kernels
            is_ = (1.0 / np.sqrt(var + eps_d)).astype(ft)
            muf = mu.astype(ft)
            sc = gm * is_
            co[g] = muf, is_, sc, bt - muf * sc
        if rm is not None:
            unbiased = var * (count / (count - 1.0)) if count > 1.0 else var
            rm = (ft(1) - m) * rm + m * muf
            rv = (ft(1) - m) * rv + m * unbiased.astype(ft)
    return co, rm, rv


def bwd_finalize(s1, s2, count, gamma, invstd, dgamma, dbeta, accumulate, local=None, ft=f32):
    """bn_bwd_finalize(_grouped)_kernel / bn_bwd_finalize_sums_kernel / the publisher of bn_bwd_fin_apply_kernel: f64 sums
    (sum dz, sum dz*xhat) [groups][C] -> dgamma, dbeta (None: not wanted), coef [groups][3][C].  Group g adds into dgamma /
    dbeta when `accumulate or g > 0`.  local: the SyncBN form -- (l1, l2) are this rank's sums (dgamma / dbeta), s1 / s2 the
    global ones with the global count (the dx coefficients)."""
    s1, s2 = np.asarray(s1, dtype=f64), np.asarray(s2, dtype=f64)
    l1, l2 = (s1, s2) if local is None else (np.asarray(local[0], dtype=f64), np.asarray(local[1], dtype=f64))
    G, C = s1.shape
    count = f64(count)
    gm = np.ones(C, ft) if gamma is None else np.asarray(gamma).astype(ft)
    dg = None if dgamma is None else np.asarray(dgamma).astype(ft)
    db = None if dbeta is None else np.asarray(dbeta).astype(ft)
    coef = np.empty((G, 3, C), ft)
    for g in range(G):
        fs1, fs2 = l1[g].astype(ft), l2[g].astype(ft)
        acc = bool(accumulate) or g > 0
        if dg is not None:
            dg = dg + fs2 if acc else fs2
        if db is not None:
            db = db + fs1 if acc else fs1
        a = gm * np.asarray(invstd[g]).astype(ft)
        coef[g] = a, (a.astype(f64) * s2[g] / count).astype(ft), (a.astype(f64) * s1[g] / count).astype(ft)
    return dg, db, coef


def eval_coeffs(gamma, beta, rmean, rvar, eps, ft=f32):
    """bn_eval_kernel -> scale, shift [C] (all in ft: the kernel works in f32)."""
    rm, rv = np.asarray(rmean).astype(ft), np.asarray(rvar).astype(ft)
    gm = np.ones(rm.size, ft) if gamma is None else np.asarray(gamma).astype(ft)
    bt = np.zeros(rm.size, ft) if beta is None else np.asarray(beta).astype(ft)
    is_ = ft(1) / np.sqrt(rv + ft(f32(eps)))
    sc = gm * is_
    return sc, bt - rm * sc


def forward(x, scale, shift, act, slope, dtype, groups=1, ft=f32):
    """y = act(scale * x + shift) as stored; scale None: the activation alone.  scale, shift [groups][C]."""
    xs = _grouped(x, groups, ft)
    z = xs if scale is None else _fma(_per_group(scale, ft), xs, _per_group(shift, ft), ft)
    return store(act_fwd(z, act, slope).reshape(np.asarray(x).shape), dtype, ft)


def apply(x, dy, coeffs, coef, act, slope, dtype, groups=1, ft=f32, zero_positive=False):
    """dx = a * dz - b * ((x - mu) * is) - c as stored, with bn_act_bwd_apply_kernel's roundings: fma(a, dz, -(b * xhat)),
    then - c."""
    xs, gs = _grouped(x, groups, ft), _grouped(dy, groups, ft)
    co, cf = np.asarray(coeffs).astype(ft), np.asarray(coef).astype(ft)
    mu, is_, sc, sh = (_per_group(co[:, k], ft) for k in range(4))
    a, b, c = (_per_group(cf[:, k], ft) for k in range(3))
    dz = act_bwd(_fma(sc, xs, sh, ft), gs, act, slope, zero_positive)
    xh = b * ((xs - mu) * is_)
    return store((_fma(a, dz, -xh, ft) - c).reshape(np.asarray(x).shape), dtype, ft)


# ---- exactness -----------------------------------------------------------------------------------------------------------
def significant_bits(a):
    """Largest number of significant bits among the values of `a` (0 for all zeros)."""
    a = np.asarray(a, dtype=f64).ravel()
    a = np.abs(a[a != 0])
    if a.size == 0:
        return 0
    m, _ = np.frexp(a)                              # m in [0.5, 1): m * 2**53 is an integer
    k = (m * 2.0 ** 53).astype(np.uint64)
    low = k & (~k + np.uint64(1))                   # lowest set bit
    return int(53 - np.log2(low.astype(f64)).min())


def fits_bf16(a):
    return significant_bits(a) <= 8 and bool((bf16_round(np.asarray(a, dtype=f32)) == np.asarray(a, dtype=f32)).all())


def sum_is_exact(terms, axis=1):
    """Every f32 partial sum of the terms along `axis`, in any order, is exact: all terms are multiples of one power of two q
    and sum |term| < 2**24 * q."""
    t = np.abs(np.asarray(terms, dtype=f64))
    nz = t[t != 0]
    if nz.size == 0:
        return True
    m, e = np.frexp(nz)
    k = (m * 2.0 ** 53).astype(np.uint64)
    low = np.log2((k & (~k + np.uint64(1))).astype(f64))
    q = 2.0 ** float((e - 53 + low).min())          # the finest quantum among the terms
    return bool(t.sum(axis).max() < 2.0 ** 24 * q)


def same_in_both(fn):
    """fn(ft) evaluated in f32 equals fn evaluated in f64, value for value: no f32 operation of the stage rounded (every
    value the reference forms survives the round trip through f32).  Works on tuples of arrays; None entries are skipped."""
    a, b = fn(f32), fn(f64)
    a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
    return all(u is None or bool((np.asarray(u, dtype=f64) == np.asarray(v, dtype=f64)).all()) for u, v in zip(a, b))


# ---- integer operands ----------------------------------------------------------------------------------------------------
# Per-(group, channel) coefficients come from short tables indexed by c + k * g with table lengths and strides chosen so
# that neighbouring channels and different groups never share an entry (every table's neighbours, wrap-around included,
# differ, and the group strides are non-zero modulo the table length for up to three groups).
_SC = np.array([0.5, -1.0, 2.0, -0.5, 1.0, -2.0])                # scale: signed powers of two
_X0 = np.array([1.0, -2.0, 3.0, -1.0, 2.0, -3.0, 4.0])           # the x at which sc * x + sh == 0: shift = -sc * x0
_MU = np.array([0.0, 0.5, -1.0, 1.5, -2.0])                      # mean: integers and halves
_IS = np.array([1.0, 2.0])                                       # invstd: positive powers of two
_A = np.array([-1.0, 2.0, -0.5, 1.0, -2.0, 0.5])                 # a: signed powers of two
_B = np.array([0.25, -0.5, -0.25, 0.5])                          # b: signed powers of two
_CC = np.array([1.0, -0.5, 2.0, -1.5, 0.5, -3.0, 1.5])           # c: integers and halves
_GAMMA = np.array([1.0, -2.0, 0.5, 2.0, -0.5, -1.0])
_BETA = np.array([0.0, 1.5, -1.0, 0.5, 2.0, -2.5, 3.0])


def _tab(tab, C, groups, stride):
    c, g = np.arange(C)[None, :], np.arange(groups)[:, None]
    return tab[(c + stride * g) % len(tab)].astype(f32)


def stream_coeffs(groups, C):
    """-> coeffs [groups][4][C], coef [groups][3][C], x0 [groups][C] (sc * x0 + sh == 0)."""
    sc, x0 = _tab(_SC, C, groups, 2), _tab(_X0, C, groups, 3)
    coeffs = np.stack([_tab(_MU, C, groups, 1), _tab(_IS, C, groups, 1), sc, -sc * x0], 1)
    coef = np.stack([_tab(_A, C, groups, 2), _tab(_B, C, groups, 1), _tab(_CC, C, groups, 3)], 1)
    return coeffs.astype(f32), coef.astype(f32), x0


def _nonzero_ints(rng, shape, hi):
    v = rng.integers(1, hi + 1, shape)
    return (v * rng.choice([-1, 1], shape)).astype(f32)


def int_stream_case(seed, rpg, groups, C, xmax=6):
    """Integer data for the column reduce and the elementwise passes, with the coefficients of stream_coeffs().
    x in +-[1, xmax], dy in +-[1, 4], drawn per element (rows and channels are not interchangeable).  Guarantees:
      z_each_channel  every (group, channel) has rows with sc*x+sh > 0, < 0 and == 0 (needs rows_per_group >= 3; with fewer
                      rows the three values are dealt over the channels instead, so the case still has each of them)
    -> dict(x, dy, coeffs, coef, z_each_channel)."""
    rng = np.random.default_rng(seed)
    x = _nonzero_ints(rng, (groups, rpg, C), xmax)
    dy = _nonzero_ints(rng, (groups, rpg, C), 4)
    coeffs, coef, x0 = stream_coeffs(groups, C)
    up = np.where(x0 + 1 == 0, 2.0, 1.0)                          # x0 + up != 0, x0 - dn != 0: the data stay non-zero
    dn = np.where(x0 - 1 == 0, 2.0, 1.0)
    three = np.stack([x0, x0 + up, x0 - dn], 0)                   # z == 0, z of sc's sign, z of the other sign
    c = np.arange(C)
    for g in range(groups):
        if rpg >= 3:
            for k in range(3):
                x[g, (c + k) % rpg, c] = three[k, g]                 # which row: varies with the channel
        else:
            for r in range(rpg):
                x[g, r, c] = three[(c + r) % 3, g, c]
    return dict(x=x.reshape(groups * rpg, C), dy=dy.reshape(groups * rpg, C), coeffs=coeffs, coef=coef,
                z_each_channel=rpg >= 3)


def _split(rng, total, nparts):
    """Integer array `total` [..., C] -> nparts uneven integer rows that add up to it."""
    parts = rng.integers(-40, 41, (nparts,) + total.shape).astype(f64)
    parts[-1] = total - parts[:-1].sum(0)
    return parts


_MEAN_INT = np.array([2.0, -1.0, 3.0, 0.0, -4.0, 1.0, -3.0])
_VPE = {0.0: np.array([0.25, 1.0, 4.0, 16.0]), 3.0: np.array([4.0, 16.0, 64.0])}      # var + eps; var = that - eps >= 0
_RM0 = np.array([0.5, -1.0, 2.0, -1.5, 0.0])
_RV0 = np.array([1.0, 0.5, 2.0, 4.0, 0.25])


def fwd_slab_case(seed, C, nparts, groups, count, eps, momentum, gamma=True, beta=True, running=True, rvar_zero=False):
    """Hand-made statistics slabs (consistent with no x): per (group, channel) an integer mean mu and a variance v with
    v + eps a power of four; count * mu and count * (mu*mu + v) are dealt unevenly over the part rows.  mean, invstd, scale
    and shift then come out as exact dyadic numbers.  count must be a multiple of 4 (v = 1/4).  See the module docstring for
    the running variance: momentum in {0.5, 1}, or rvar_zero with one group.
    -> dict(slabs [groups][nparts][2][C] f32, count, eps, momentum, gamma, beta, rmean, rvar)."""
    assert count % 4 == 0 and (momentum in (0.5, 1.0) or (rvar_zero and groups == 1))
    rng = np.random.default_rng(seed)
    mu = _tab(_MEAN_INT, C, groups, 3).astype(f64)
    v = _tab(_VPE[float(eps)], C, groups, 1).astype(f64) - float(eps)
    s1, s2 = count * mu, count * (mu * mu + v)
    slabs = np.empty((groups, nparts, 2, C), f64)
    slabs[:, :, 0] = np.moveaxis(_split(rng, s1, nparts), 0, 1)
    slabs[:, :, 1] = np.moveaxis(_split(rng, s2, nparts), 0, 1)
    assert (slabs == np.round(slabs)).all() and np.abs(slabs).max() < 2 ** 24
    one = lambda tab: _tab(tab, C, 1, 0)[0]
    return dict(slabs=slabs.astype(f32), count=count, eps=float(eps), momentum=float(momentum),
                gamma=one(_GAMMA) if gamma else None, beta=one(_BETA) if beta else None,
                rmean=one(_RM0) if running else None,
                rvar=(np.zeros(C, f32) if rvar_zero else one(_RV0)) if running else None)


def eval_case(C, eps):
    """Running statistics for eval mode: running_var + eps a power of four, running_mean integers and halves."""
    return _tab(_RM0, C, 1, 0)[0], (_tab(_VPE[float(eps)], C, 1, 0)[0] - f32(eps)).astype(f32)


_T = np.array([2.0, -1.0, 3.0, -2.0, 1.0, -3.0, 4.0])
_DG0 = np.array([1.0, -2.5, 3.0, 0.5, -1.0])


def bwd_slab_case(seed, C, nparts, groups, count, gamma=True, grads=True, coef=None):
    """Hand-made backward slabs: sum dz = count * t1, sum dz*xhat = count * t2 with small integers t, dealt unevenly over the
    part rows; gamma and invstd are powers of two, so a = gamma * invstd, b = a * t2 and c = a * t1 are exact.  coef
    [groups][3][C]: choose the sums so that b and c come out as THESE values instead (for the fused backward, whose dx must be
    exact too; count * coef / a must be integers).
    -> dict(slabs, count, gamma, invstd [groups][C], dgamma, dbeta (initial values))."""
    rng = np.random.default_rng(seed)
    gm = _tab(_GAMMA, C, 1, 0)[0] if gamma else None
    invstd = _tab(_IS, C, groups, 1)
    a = (np.ones(C, f32) if gm is None else gm)[None, :] * invstd
    if coef is None:
        t1, t2 = _tab(_T, C, groups, 3).astype(f64), _tab(_T, C, groups, 2)[:, ::-1].astype(f64)
    else:
        t1, t2 = coef[:, 2].astype(f64) / a, coef[:, 1].astype(f64) / a
    s1, s2 = count * t1, count * t2
    slabs = np.empty((groups, nparts, 2, C), f64)
    slabs[:, :, 0] = np.moveaxis(_split(rng, s1, nparts), 0, 1)
    slabs[:, :, 1] = np.moveaxis(_split(rng, s2, nparts), 0, 1)
    assert (slabs == np.round(slabs)).all() and np.abs(slabs).max() < 2 ** 24, "count * t must be integers"
    one = lambda tab: _tab(tab, C, 1, 0)[0]
    return dict(slabs=slabs.astype(f32), count=count, gamma=gm, invstd=invstd,
                dgamma=one(_DG0) if grads else None, dbeta=one(_DG0[::-1].copy()) if grads else None)


_AMP = np.array([0.5, 1.0, 2.0, 4.0])


def two_point_case(seed, rpg, groups, C):
    """Data whose statistics are exact: per (group, channel) half the rows at m + a and half at m - a (a power of two, m an
    integer), permuted over the rows, so that mean = m, var = a*a, invstd = 1 / a with eps = 0.  rows_per_group a power of two
    keeps the backward coefficients a * sum / count dyadic as well.  beta = gamma on every third channel puts half of its
    rows at z == 0 exactly (xhat = +-1, so z = +-gamma + beta).
    -> dict(x, dy, gamma, beta, rmean, rvar, momentum, eps)."""
    assert rpg >= 2 and rpg & (rpg - 1) == 0
    rng = np.random.default_rng(seed)
    m, amp = _tab(_MEAN_INT, C, groups, 3), _tab(_AMP, C, groups, 1)
    sign = np.where(np.arange(rpg) % 2 == 0, 1.0, -1.0).astype(f32)
    sign = np.stack([rng.permuted(np.tile(sign[:, None], (1, C)), axis=0) for _ in range(groups)])
    x = m[:, None, :] + sign * amp[:, None, :]
    gamma = _tab(_GAMMA, C, 1, 0)[0]
    beta = np.where(np.arange(C) % 3 == 0, gamma, _tab(_BETA, C, 1, 0)[0]).astype(f32)
    return dict(x=x.reshape(groups * rpg, C).astype(f32), dy=_nonzero_ints(rng, (groups * rpg, C), 4), gamma=gamma, beta=beta,
                rmean=_tab(_RM0, C, 1, 0)[0], rvar=_tab(_RV0, C, 1, 0)[0], momentum=0.5, eps=0.0)


# ---- case tables ---------------------------------------------------------------------------------------------------------
# The three forms of the streaming kernels: f32, bf16 as shipped (8-byte vectors below VG_BN_WIDE_MIN) and bf16 with the
# 16-byte vectors of the large tensors forced (VG_BN_WIDE_MIN=0; taken where C % 8 == 0).
MODES = {"f32": (F32, None), "bf16": (BF16, None), "bf16_wide": (BF16, 0)}

# name, rows per group, groups, C, act, slope, modes, kinds.  The first nine are the shapes of tools/gen_golden_bn_stream.py
# (chosen for the thread mapping); the rest is what that table lacks.  Slopes are powers of two.
ALL, RFA = ("f32", "bf16", "bf16_wide"), ("reduce", "forward", "apply")
STREAM_CASES = [
    ("c4", 35, 1, 4, ACT_RELU, 0.0, ALL, RFA),                    # 1 thread per row
    ("c36", 35, 1, 36, ACT_LRELU, 0.5, ALL, RFA),                 # 9 threads per row, 28 rows per pass, 4 threads idle
    ("c8_row1", 1, 1, 8, ACT_NONE, 0.0, ALL, RFA),                # a single row
    ("c8_ragged", 600, 1, 8, ACT_LRELU, 0.25, ALL, RFA),          # several workgroups and a ragged last one
    ("c200", 23, 1, 200, ACT_LRELU, 0.5, ALL, RFA),               # 25 / 50 threads per row, idle threads, ragged last pass
    ("c200_g3", 7, 3, 200, ACT_RELU, 0.0, ALL, RFA),              # three groups, fewer rows than one pass
    ("c64_g2", 45, 2, 64, ACT_LRELU, 0.25, ALL, RFA),             # two groups
    ("c1024_g2", 3, 2, 1024, ACT_RELU, 0.0, ALL, RFA),            # 2 rows per pass (wide), 3 rows per group
    ("c4096", 3, 1, 4096, ACT_NONE, 0.0, ALL, ("forward", "apply")),   # 4 (narrow) / 2 (wide) column blocks
    ("c200_parts", 83, 1, 200, ACT_LRELU, 0.25, ("f32", "bf16"), ("reduce",)),     # 2 parts of 45 rows, the last one short
    ("c1024_clip_g2", 37, 2, 1024, ACT_LRELU, 0.5, ("f32", "bf16"), ("reduce",)),  # 4 parts of 10 rows: the 4th clipped by its group
    ("c1040", 70, 1, 1040, ACT_LRELU, 0.5, ALL, RFA),             # reduce: 2nd column block of 4 columns, 64 rows per pass
    ("c1024_trips_w", 10243, 1, 1024, ACT_LRELU, 0.25, ("bf16_wide",), ("forward", "apply")),   # past the workgroup cap
    ("c1024_trips", 6147, 1, 1024, ACT_RELU, 0.0, ("f32",), ("forward", "apply")),
    ("c1024_tail1", 4100, 1, 1024, ACT_LRELU, 0.5, ("f32",), ("forward", "apply")),
]


def case_seed(name):
    return 4100 + 7 * [c[0] for c in STREAM_CASES].index(name)


def stream_params():
    """(case, mode, kind) for every cell of the table: the parametrisation of the streaming tests."""
    return [(c, m, k) for c in STREAM_CASES for m in c[6] for k in c[7]]


# hand-made slabs for the finalize kernels: nparts x C (the short loop, the plane stride of 128, the four-deep unrolled loop
# from 4 * 128 + 1 rows on; C = 12 leaves the second 8-channel workgroup half empty).  The options cycle with the case index.
FIN_NPARTS, FIN_C = (1, 127, 129, 513, 1300), (4, 12, 200, 1024)
FIN_CASES = [(n, c) for n in FIN_NPARTS for c in FIN_C]


def fin_options(i):
    """gamma / beta present, running statistics present, accumulate, dgamma / dbeta present, groups, eps -- every value of
    each with every kernel over the 20 cases."""
    return dict(affine=i % 2 == 0, running=i % 3 != 1, accumulate=i % 4 in (1, 2), grads=i % 5 != 3,
                groups=1 + i % 3, eps=(0.0, 3.0)[(i // 2) % 2], momentum=(0.5, 1.0)[(i // 3) % 2])


# the one-launch forms: name, rows per group, groups, C, slab rows per group, act, slope
FUSED_CASES = [
    ("f64_g1", 144, 1, 64, 3, ACT_LRELU, 0.25),                   # 2 row blocks of 128 rows, the second 16 rows long
    ("f64_g2", 144, 2, 64, 17, ACT_RELU, 0.0),                    # two groups: the publisher walks both; blocks clipped by a group
    ("f128_g2", 1008, 2, 128, 200, ACT_LRELU, 0.5),               # the largest slab the form takes, 2 channel slices
    ("f256_g1", 48, 1, 256, 1, ACT_NONE, 0.0),                    # fewer rows than one pass, 4 slices, one slab row
]
# (rows per group, groups, C, slab rows): refused by C % 64, by slab rows > 200 and by size (> 9 MiB), each next to the
# nearest shape that is taken (rows per group are multiples of 16: bwd_slab_case's count * coef / a must be integers)
FUSED_REFUSED = {"c_mod_64": ((144, 1, 96, 3), (144, 1, 64, 3)), "slab_rows": ((144, 1, 64, 201), (144, 1, 64, 200)),
                 "bytes": ((4616, 1, 1024, 8), (4608, 1, 1024, 8))}
# the chain on two-point data: rows per group (a power of two), groups, C, act, slope
CHAIN_CASES = [("ch64_g1", 256, 1, 64, ACT_LRELU, 0.25), ("ch128_g2", 512, 2, 128, ACT_LRELU, 0.5),
               ("ch200_g2", 64, 2, 200, ACT_RELU, 0.0)]


# ---- inputs and references shared by the CPU and the GPU tests ------------------------------------------------------------
def fused_inputs(case):
    """x, dy, hand-made forward slabs (count = rows per group), coefficients and backward slabs whose b, c are the stream
    table's."""
    name, rpg, groups, C, nparts, act, slope = case
    seed = 900 + [c[0] for c in FUSED_CASES].index(name)
    d = int_stream_case(seed, rpg, groups, C)
    fw = fwd_slab_case(seed, C, nparts, groups, rpg, 0.0, 0.5)
    bw = bwd_slab_case(seed + 50, C, nparts, groups, rpg, coef=d["coef"])
    return d, fw, bw


def chain_inputs(case):
    name, rpg, groups, C, act, slope = case
    return two_point_case(1000 + rpg + C, rpg, groups, C)


def chain_ref(d, rpg, groups, C, act, slope, dtype, ft=f32):
    """stats -> finalize -> forward -> reduce -> bwd-finalize -> apply on two-point data."""
    s1, s2 = col_stats(d["x"], groups, ft)
    co, rm, rv = finalize(s1, s2, rpg, d["gamma"], d["beta"], d["rmean"], d["rvar"], d["momentum"], d["eps"], ft)
    y = forward(d["x"], co[:, 2], co[:, 3], act, slope, dtype, groups, ft)
    b1, b2 = bwd_sums(d["x"], d["dy"], co, act, slope, groups, ft)
    dg, db, cf = bwd_finalize(b1, b2, rpg, d["gamma"], co[:, 1], np.zeros(C, f32), np.zeros(C, f32), False, ft=ft)
    dx = apply(d["x"], d["dy"], co, cf, act, slope, dtype, groups, ft)
    return dict(stats=(s1, s2), coeffs=co, rmean=rm, rvar=rv, y=y, partial=(b1, b2), dgamma=dg, dbeta=db, coef=cf, dx=dx)
