"""GPU: every BatchNorm entry point of csrc/bn_act.hip against the numpy restatement of tests/_bn_ref.py, bit for bit.

The operands are integers, powers of two and halves on which every intermediate is exactly representable (conditions and
blind spots of every case: tests/test_bn_cpu.py), so the reference is unique and every comparison is torch.equal on the raw
bits -- whether a kernel contracts a multiply-add or not, and in whichever order it sums.  Destinations are NaN-filled and
sit between sentinel rows that must still be NaN afterwards.  The C ABI is called directly (ops.py hides outputs).  The only
toleranced assertions are those of test_finalize_on_float_slabs_within_the_rounding_bound, whose bound is derived there.
"""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import _bn_ref as R

pytestmark = pytest.mark.gpu

PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
DEV = "cuda"
f32, f64 = np.float32, np.float64
TD = {R.F32: torch.float32, R.BF16: torch.bfloat16}
BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float64: torch.int64, torch.uint8: torch.uint8}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module(PKG + ".ops")


@pytest.fixture(scope="module")
def L():
    return importlib.import_module(PKG + "._lib")


@pytest.fixture
def separate(vg_switch):
    vg_switch("VG_BN_FUSED_FWD", 0)
    vg_switch("VG_BN_ONEPASS", 0)


def dev(a, td=torch.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(td).to(DEV)


class Out:
    """A destination of `shape` between two sentinel regions of two rows of the last axis each (one [2][C] slab row), all
    NaN (0xA5 bytes)."""

    def __init__(self, shape, td=torch.float32):
        self.n = int(np.prod(shape))
        self.pad = -(-max(2 * shape[-1], 16) // 16) * 16                 # a multiple of 16 elements: keeps 16-byte alignment
        self.buf = torch.empty(self.n + 2 * self.pad, dtype=td, device=DEV)
        self.buf.fill_(0xA5 if td == torch.uint8 else float("nan"))
        self.t = self.buf[self.pad:self.pad + self.n].view(*shape)

    def ptr(self, offset=0):
        return self.t.data_ptr() + offset * self.t.element_size()

    def sentinels_intact(self):
        edge = torch.cat([self.buf[:self.pad], self.buf[self.pad + self.n:]])
        return bool((edge == 0xA5).all() if edge.dtype == torch.uint8 else torch.isnan(edge).all())


def assert_bits(out, want, what):
    """out: Out or tensor; want: numpy reference holding exactly representable values of the tensor's dtype."""
    t = out.t if isinstance(out, Out) else out
    have = t.detach().cpu().contiguous()
    ref = torch.from_numpy(np.ascontiguousarray(want))
    ref = ref.to(have.dtype).reshape(have.shape)
    assert torch.equal(ref.double(), torch.from_numpy(np.ascontiguousarray(want)).double().reshape(have.shape)), what + ": reference not representable"
    hb, rb = have.view(BITS[have.dtype]), ref.view(BITS[have.dtype])
    if not torch.equal(hb, rb):
        bad = (hb != rb).flatten().nonzero().flatten()
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of {hb.numel()} words differ; first at flat index {i}: "
                             f"got {have.flatten()[i].item()!r}, want {ref.flatten()[i].item()!r}")
    if isinstance(out, Out):
        assert out.sentinels_intact(), what + ": wrote outside its rows"


def check(L, rc, what):
    L.check(rc, what)


def _stream_setup(vg_switch, ops, case, mode, kind):
    name, rpg, groups, C, act, slope = case[:6]
    dtype, wide_min = R.MODES[mode]
    if wide_min is not None:
        vg_switch("VG_BN_WIDE_MIN", wide_min)
    d = R.int_stream_case(R.case_seed(name), rpg, groups, C, xmax=20 if kind == "forward" else 6)
    return rpg, groups, C, act, slope, dtype, d, dev(d["x"], TD[dtype]), dev(d["dy"], TD[dtype]), dev(d["coeffs"]), dev(d["coef"])


def _ids(params):
    return [f"{c[0]}-{m}" for c, m in params]


# the column reduce has one form per dtype (4 channels per thread): VG_BN_WIDE_MIN does not reach it
REDUCE = [(c, m) for c, m, k in R.stream_params() if k == "reduce" and m != "bf16_wide"]
FORWARD = [(c, m) for c, m, k in R.stream_params() if k == "forward"]
APPLY = [(c, m) for c, m, k in R.stream_params() if k == "apply"]


# ---- column reduces -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,mode", REDUCE, ids=_ids(REDUCE))
def test_column_reduces(ops, L, separate, vg_switch, case, mode):
    """vg_channel_stats (one call per group: it has no groups) and vg_bn_act_backward_reduce (one grouped launch): every part
    row against the restatement on that part's rows, and the parts summed against the restatement on the group."""
    rpg, groups, C, act, slope, dtype, d, X, DY, CO, _ = _stream_setup(vg_switch, ops, case, mode, "reduce")
    lib = L.load()
    plan = ops.bn_launch_plan("reduce", rpg * groups, C, dtype, groups)
    nparts, rows_pp = plan["blocks_per_group"], plan["rows_per_block"]
    assert ops.bn_launch_plan("reduce", rpg, C, dtype, 1)["blocks_per_group"] == nparts
    stats, partial = Out((groups, nparts, 2, C)), Out((groups, nparts, 2, C))
    n = ctypes.c_int(0)
    for g in range(groups):
        check(L, lib.vg_channel_stats(X[g * rpg:].data_ptr(), rpg, C, stats.ptr(g * nparts * 2 * C), nparts, ctypes.byref(n),
                                      dtype, L.stream_ptr()), "vg_channel_stats")
        assert n.value == nparts
    check(L, lib.vg_bn_act_backward_reduce(X.data_ptr(), DY.data_ptr(), CO[0, 2].data_ptr(), CO[0, 3].data_ptr(),
                                           CO[0, 0].data_ptr(), CO[0, 1].data_ptr(), rpg * groups, C, act, slope, partial.ptr(),
                                           nparts * groups, ctypes.byref(n), groups, 4 * C, dtype, L.stream_ptr()),
          "vg_bn_act_backward_reduce")
    assert n.value == nparts
    want_stats, want_partial = np.empty((groups, nparts, 2, C), f32), np.empty((groups, nparts, 2, C), f32)
    for g in range(groups):
        for p in range(nparts):
            lo = g * rpg + p * rows_pp
            hi = min((g + 1) * rpg, lo + rows_pp)
            want_stats[g, p] = np.stack([s[0] for s in R.col_stats(d["x"][lo:hi])])
            want_partial[g, p] = np.stack([s[0] for s in R.bwd_sums(d["x"][lo:hi], d["dy"][lo:hi], d["coeffs"][g:g + 1], act, slope)])
    assert_bits(stats, want_stats, "vg_channel_stats parts")
    assert_bits(partial, want_partial, "vg_bn_act_backward_reduce parts")
    whole = np.stack(R.col_stats(d["x"], groups), 1), np.stack(R.bwd_sums(d["x"], d["dy"], d["coeffs"], act, slope, groups), 1)
    assert_bits(stats.t.double().sum(1).float(), whole[0], "vg_channel_stats summed over parts")
    assert_bits(partial.t.double().sum(1).float(), whole[1], "vg_bn_act_backward_reduce summed over parts")


# ---- elementwise passes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,mode", FORWARD, ids=_ids(FORWARD))
def test_forward(ops, L, separate, vg_switch, case, mode):
    """vg_bn_act_forward, vg_bn_act_forward_fp8 (bf16: y again and its e4m3 twin) and the coefficient-free mode."""
    rpg, groups, C, act, slope, dtype, d, X, _, CO, _ = _stream_setup(vg_switch, ops, case, mode, "forward")
    lib, rows, td = L.load(), rpg * groups, TD[dtype]
    assert ops.bn_launch_plan("forward", rows, C, dtype, groups)["vec"] == (8 if mode == "bf16_wide" and C % 8 == 0 else 4)
    want = R.forward(d["x"], d["coeffs"][:, 2], d["coeffs"][:, 3], act, slope, dtype, groups)
    y = Out((rows, C), td)
    check(L, lib.vg_bn_act_forward(X.data_ptr(), y.ptr(), CO[0, 2].data_ptr(), CO[0, 3].data_ptr(), rows, C, act, slope, groups,
                                   4 * C, dtype, L.stream_ptr()), "vg_bn_act_forward")
    assert_bits(y, want, "vg_bn_act_forward")
    if dtype == R.BF16:
        y2, y8 = Out((rows, C), td), Out((rows, C), torch.uint8)
        check(L, lib.vg_bn_act_forward_fp8(X.data_ptr(), y2.ptr(), y8.ptr(), CO[0, 2].data_ptr(), CO[0, 3].data_ptr(), rows, C,
                                           act, slope, groups, 4 * C, dtype, L.stream_ptr()), "vg_bn_act_forward_fp8")
        assert_bits(y2, want, "vg_bn_act_forward_fp8 y")
        assert_bits(y8, R.e4m3_twin(want), "vg_bn_act_forward_fp8 twin")
    ya = Out((rows, C), td)
    check(L, lib.vg_bn_act_forward(X.data_ptr(), ya.ptr(), None, None, rows, C, R.ACT_LRELU, 0.25, 1, 0, dtype, L.stream_ptr()),
          "vg_bn_act_forward (activation only)")
    assert_bits(ya, R.forward(d["x"], None, None, R.ACT_LRELU, 0.25, dtype), "activation-only forward")


@pytest.mark.parametrize("case,mode", APPLY, ids=_ids(APPLY))
def test_backward_apply(ops, L, separate, vg_switch, case, mode):
    rpg, groups, C, act, slope, dtype, d, X, DY, CO, CF = _stream_setup(vg_switch, ops, case, mode, "apply")
    lib, rows = L.load(), rpg * groups
    assert ops.bn_launch_plan("apply", rows, C, dtype, groups)["vec"] == (8 if mode == "bf16_wide" and C % 8 == 0 else 4)
    dx = Out((rows, C), TD[dtype])
    check(L, lib.vg_bn_act_backward_apply(X.data_ptr(), DY.data_ptr(), dx.ptr(), CO[0, 2].data_ptr(), CO[0, 3].data_ptr(),
                                          CO[0, 0].data_ptr(), CO[0, 1].data_ptr(), CF.data_ptr(), rows, C, act, slope, groups,
                                          4 * C, 3 * C, dtype, L.stream_ptr()), "vg_bn_act_backward_apply")
    assert_bits(dx, R.apply(d["x"], d["dy"], d["coeffs"], d["coef"], act, slope, dtype, groups), "vg_bn_act_backward_apply")


# ---- finalize kernels on hand-made slabs -----------------------------------------------------------------------------------
def _p(t):
    return None if t is None else t.ptr() if isinstance(t, Out) else t.data_ptr()


def _running(fw):
    """Fresh device copies of the initial running statistics, between sentinels."""
    if fw["rmean"] is None:
        return None, None
    rm, rv = Out((fw["rmean"].size,)), Out((fw["rmean"].size,))
    rm.t.copy_(dev(fw["rmean"])), rv.t.copy_(dev(fw["rvar"]))
    return rm, rv


def _grads(bw):
    if bw["dgamma"] is None:
        return None, None
    dg, db = Out((bw["dgamma"].size,)), Out((bw["dgamma"].size,))
    dg.t.copy_(dev(bw["dgamma"])), db.t.copy_(dev(bw["dbeta"]))
    return dg, db


@pytest.mark.parametrize("i", range(len(R.FIN_CASES)), ids=[f"n{n}_c{c}" for n, c in R.FIN_CASES])
def test_finalize_kernels_on_hand_made_slabs(ops, L, i):
    """vg_bn_finalize, _grouped, vg_slab_sums + vg_bn_finalize_sums, vg_bn_backward_finalize, _grouped, _sums and
    vg_bn_eval_coeffs; options (affine, running statistics, accumulate, dgamma / dbeta, groups, eps, momentum) by case."""
    nparts, C = R.FIN_CASES[i]
    o = R.fin_options(i)
    G, count, acc = o["groups"], 4 * (9 + i), int(o["accumulate"])
    fw = R.fwd_slab_case(700 + i, C, nparts, G, count, o["eps"], o["momentum"], gamma=o["affine"], beta=o["affine"],
                         running=o["running"])
    bw = R.bwd_slab_case(800 + i, C, nparts, G, count, gamma=o["affine"], grads=o["grads"])
    lib, sp = L.load(), L.stream_ptr()
    S, gm, bt = dev(fw["slabs"]), dev(fw["gamma"]), dev(fw["beta"])
    s1, s2 = R.slab_sums(fw["slabs"])
    mom, eps = fw["momentum"], fw["eps"]
    # forward, one group: group 0 alone
    co1, rm1, rv1 = R.finalize(s1[:1], s2[:1], count, fw["gamma"], fw["beta"], fw["rmean"], fw["rvar"], mom, eps)
    rm, rv = _running(fw)
    co = Out((1, 4, C))
    check(L, lib.vg_bn_finalize(S.data_ptr(), nparts, C, count, L.ptr(gm), L.ptr(bt), _p(rm), _p(rv), mom, eps, co.ptr(),
                                co.ptr(C), co.ptr(2 * C), co.ptr(3 * C), sp), "vg_bn_finalize")
    assert_bits(co, co1, "vg_bn_finalize coefficients")
    if rm is not None:
        assert_bits(rm, rm1, "vg_bn_finalize running mean"), assert_bits(rv, rv1, "vg_bn_finalize running var")
    # forward, grouped
    coG, rmG, rvG = R.finalize(s1, s2, count, fw["gamma"], fw["beta"], fw["rmean"], fw["rvar"], mom, eps)
    rm, rv = _running(fw)
    co = Out((G, 4, C))
    check(L, lib.vg_bn_finalize_grouped(S.data_ptr(), nparts, G, C, count, L.ptr(gm), L.ptr(bt), _p(rm), _p(rv), mom, eps,
                                        co.ptr(), sp), "vg_bn_finalize_grouped")
    assert_bits(co, coG, "vg_bn_finalize_grouped coefficients")
    if rm is not None:
        assert_bits(rm, rmG, "grouped running mean"), assert_bits(rv, rvG, "grouped running var")
    # SyncBN: f64 sums, then the finalize from sums group after group on the same running statistics
    sums = Out((G, 2, C), torch.float64)
    rm, rv = _running(fw)
    co = Out((G, 4, C))
    for g in range(G):
        check(L, lib.vg_slab_sums(S[g].data_ptr(), nparts, C, sums.ptr(g * 2 * C), sp), "vg_slab_sums")
        check(L, lib.vg_bn_finalize_sums(sums.ptr(g * 2 * C), C, count, L.ptr(gm), L.ptr(bt), _p(rm), _p(rv), mom, eps,
                                         co.ptr(g * 4 * C), co.ptr(g * 4 * C + C), co.ptr(g * 4 * C + 2 * C),
                                         co.ptr(g * 4 * C + 3 * C), sp), "vg_bn_finalize_sums")
    assert_bits(sums, np.stack([s1, s2], 1), "vg_slab_sums")
    assert_bits(co, coG, "vg_bn_finalize_sums coefficients")
    if rm is not None:
        assert_bits(rm, rmG, "sums running mean"), assert_bits(rv, rvG, "sums running var")
    # backward
    P, gmb, IS = dev(bw["slabs"]), dev(bw["gamma"]), dev(bw["invstd"])
    b1, b2 = R.slab_sums(bw["slabs"])
    coeffs = torch.zeros(G, 4, C, device=DEV)
    coeffs[:, 1] = IS
    want = R.bwd_finalize(b1[:1], b2[:1], count, bw["gamma"], bw["invstd"][:1], bw["dgamma"], bw["dbeta"], acc)
    dg, db = _grads(bw)
    cf = Out((1, 3, C))
    check(L, lib.vg_bn_backward_finalize(P.data_ptr(), nparts, C, count, L.ptr(gmb), IS[0].data_ptr(), _p(dg), _p(db), acc,
                                         cf.ptr(), sp), "vg_bn_backward_finalize")
    assert_bits(cf, want[2], "vg_bn_backward_finalize coef")
    if dg is not None:
        assert_bits(dg, want[0], "vg_bn_backward_finalize dgamma"), assert_bits(db, want[1], "vg_bn_backward_finalize dbeta")
    want = R.bwd_finalize(b1, b2, count, bw["gamma"], bw["invstd"], bw["dgamma"], bw["dbeta"], acc)
    dg, db = _grads(bw)
    cf = Out((G, 3, C))
    check(L, lib.vg_bn_backward_finalize_grouped(P.data_ptr(), nparts, G, C, count, L.ptr(gmb), coeffs.data_ptr(), _p(dg), _p(db),
                                                 acc, cf.ptr(), sp), "vg_bn_backward_finalize_grouped")
    assert_bits(cf, want[2], "vg_bn_backward_finalize_grouped coef")
    if dg is not None:
        assert_bits(dg, want[0], "grouped dgamma"), assert_bits(db, want[1], "grouped dbeta")
    # SyncBN backward: two ranks with these same local sums -> global sums and count doubled; dgamma / dbeta stay local
    want = R.bwd_finalize(2 * b1, 2 * b2, 2 * count, bw["gamma"], bw["invstd"], bw["dgamma"], bw["dbeta"], acc, local=(b1, b2))
    dg, db = _grads(bw)
    cf = Out((G, 3, C))
    lsum = dev(np.stack([b1, b2], 1), torch.float64)
    gsum = 2 * lsum
    for g in range(G):
        check(L, lib.vg_bn_backward_finalize_sums(gsum[g].data_ptr(), lsum[g].data_ptr(), C, 2 * count, L.ptr(gmb),
                                                  IS[g].data_ptr(), _p(dg), _p(db), 1 if (acc or g > 0) else 0,
                                                  cf.ptr(g * 3 * C), sp), "vg_bn_backward_finalize_sums")
    assert_bits(cf, want[2], "vg_bn_backward_finalize_sums coef")
    if dg is not None:
        assert_bits(dg, want[0], "sums dgamma"), assert_bits(db, want[1], "sums dbeta")
    # eval mode: running variance + eps a power of four
    rmean, rvar = R.eval_case(C, eps)
    sc, sh = R.eval_coeffs(fw["gamma"], fw["beta"], rmean, rvar, eps)
    ev, RM, RV = Out((2, C)), dev(rmean), dev(rvar)
    check(L, lib.vg_bn_eval_coeffs(L.ptr(gm), L.ptr(bt), RM.data_ptr(), RV.data_ptr(), eps, C, ev.ptr(), ev.ptr(C), sp),
          "vg_bn_eval_coeffs")
    assert_bits(ev, np.stack([sc, sh]), "vg_bn_eval_coeffs")


U = 2.0 ** -24          # one f32 rounding, relative
S64 = 1e-11             # f64 noise: the kernels' sums of <= 1300 positive terms in another order than numpy's


def test_finalize_on_float_slabs_within_the_rounding_bound(ops, L, capsys):
    """Random non-integer slabs through the finalize kernels against the restatement in f64 WITHOUT its f32 casts.

    The bound counts the f32 roundings a kernel performs on the way to each output; u = 2^-24 is one rounding to nearest,
    relative to the rounded value, and every bound carries a factor (1 + 2^-10) for the products of two such errors.  The
    kernels' f64 work (sums of <= 1300 POSITIVE slab entries, var = s2/count - mu^2 with var ~ mu^2: no cancellation) differs
    from numpy's by the summation order only: <= 1300 * 2^-53 * 4 < 1e-12 relative, entered as S64 = 1e-11.
      mean, invstd           (float) of an f64 value: 1 rounding                      (u + S64) |ref|
      scale = g * is         is rounded, then the product: 2                          (2u + S64) |ref|
      shift = b - muf * sc   muf (1) and sc (2) rounded, the product rounded (absent when contracted): 4 on |mu * sc|,
                             then the difference: 1 on |shift|                        4u |mu sc| + u |ref| + S64 (|mu sc| + |b|)
      running mean           1 - m is rounded (m = f32(0.1)), (1-m) * rm rounded: 2 on |(1-m) rm|; muf rounded, m * muf
                             rounded: 2 on |m mu|; the sum: 1                         2u (|(1-m) rm| + |m mu|) + u |ref| + S64 |ref|
      running var            the same with (float) unbiased for muf
      coef a = g * is        both f32 inputs: 1                                       u |ref|
      coef b, c              a rounded (1), (float) of the f64 quotient (1): 2        (2u + S64) |ref|
      dgamma, dbeta          (float) of the f64 sum (1), the f32 add into the initial value when accumulating (1)
                                                                                      u |sum| + u |ref| + S64 |sum|
    The largest observed error / bound per output is printed (pytest -s) and recorded in the pull request that added the
    test; the bound was written down first."""
    nparts, C, G, count, mom, eps = 1300, 200, 2, 1300 * 37, 0.1, 1e-5
    rng = np.random.default_rng(77)
    slabs = np.empty((G, nparts, 2, C), f32)
    slabs[:, :, 0] = rng.uniform(20.0, 50.0, (G, nparts, C))              # count * mu,            mu  ~ 0.95
    slabs[:, :, 1] = rng.uniform(60.0, 120.0, (G, nparts, C))             # count * (mu^2 + var),  var ~ 1.5
    gamma, beta = rng.normal(1.0, 0.3, C).astype(f32), rng.normal(0.0, 0.5, C).astype(f32)
    rm0, rv0 = rng.normal(0.0, 1.0, C).astype(f32), rng.uniform(0.5, 2.0, C).astype(f32)
    s1, s2 = R.slab_sums(slabs)
    co64, rm64, rv64 = R.finalize(s1, s2, count, gamma, beta, rm0, rv0, mom, eps, f64)
    slack, m, one_m = 1 + 2.0 ** -10, f64(f32(mom)), 1.0 - f64(f32(mom))
    mu, is_, sc, sh = (co64[:, k] for k in range(4))
    # the running statistics after each group, for their bound (terms of the LAST update; earlier errors pass through (1-m))
    bound = {"mean": (U + S64) * np.abs(mu), "invstd": (U + S64) * np.abs(is_), "scale": (2 * U + S64) * np.abs(sc),
             "shift": 4 * U * np.abs(mu * sc) + U * np.abs(sh) + S64 * (np.abs(mu * sc) + np.abs(beta))}
    lib, sp = L.load(), L.stream_ptr()
    rm, rv, co = Out((C,)), Out((C,)), Out((G, 4, C))
    rm.t.copy_(dev(rm0)), rv.t.copy_(dev(rv0))
    S, gm, bt = dev(slabs), dev(gamma), dev(beta)                         # named: a temporary's memory is reused at once
    check(L, lib.vg_bn_finalize_grouped(S.data_ptr(), nparts, G, C, count, gm.data_ptr(), bt.data_ptr(), rm.ptr(), rv.ptr(), mom,
                                        eps, co.ptr(), sp), "vg_bn_finalize_grouped")
    got = co.t.cpu().double().numpy()
    ratios = {}
    for k, name in enumerate(("mean", "invstd", "scale", "shift")):
        err = np.abs(got[:, k] - co64[:, k])
        ratios[name] = float((err / (bound[name] * slack)).max())
    # running statistics: two updates; the error of the first passes through (1 - m) <= 1 into the second
    var = np.maximum(s2 / count - (s1 / count) ** 2, 0.0)
    unb = var * (count / (count - 1.0))
    r1m, r1v = one_m * rm0 + m * mu[0], one_m * rv0 + m * unb[0]
    step = lambda prev, new, res: 2 * U * (np.abs(one_m * prev) + np.abs(m * new)) + (U + S64) * np.abs(res)
    b_rm = step(rm0, mu[0], r1m) + step(r1m, mu[1], rm64)
    b_rv = step(rv0, unb[0], r1v) + step(r1v, unb[1], rv64)
    ratios["running_mean"] = float((np.abs(rm.t.cpu().double().numpy() - rm64) / (b_rm * slack)).max())
    ratios["running_var"] = float((np.abs(rv.t.cpu().double().numpy() - rv64) / (b_rv * slack)).max())
    assert co.sentinels_intact() and rm.sentinels_intact() and rv.sentinels_intact()
    # backward: the same slabs read as (sum dz, sum dz * xhat); invstd an f32 input
    invstd = rng.uniform(0.5, 2.0, (G, C)).astype(f32)
    dg0, db0 = rng.normal(0, 30.0, C).astype(f32), rng.normal(0, 30.0, C).astype(f32)
    dg64, db64, cf64 = R.bwd_finalize(s1, s2, count, gamma, invstd, dg0, db0, True, ft=f64)
    coeffs = torch.zeros(G, 4, C, device=DEV)
    coeffs[:, 1] = dev(invstd)
    dg, db, cf = Out((C,)), Out((C,)), Out((G, 3, C))
    dg.t.copy_(dev(dg0)), db.t.copy_(dev(db0))
    check(L, lib.vg_bn_backward_finalize_grouped(S.data_ptr(), nparts, G, C, count, gm.data_ptr(), coeffs.data_ptr(), dg.ptr(),
                                                 db.ptr(), 1, cf.ptr(), sp),
          "vg_bn_backward_finalize_grouped")
    gcf = cf.t.cpu().double().numpy()
    ratios["coef_a"] = float((np.abs(gcf[:, 0] - cf64[:, 0]) / (U * np.abs(cf64[:, 0]) * slack)).max())
    for k, name in ((1, "coef_b"), (2, "coef_c")):
        ratios[name] = float((np.abs(gcf[:, k] - cf64[:, k]) / ((2 * U + S64) * np.abs(cf64[:, k]) * slack)).max())
    # dgamma = (dg0 + f32(s2[0])) + f32(s2[1]): per group one cast of the sum and one add
    for name, out, ref, s, init in (("dgamma", dg, dg64, s2, dg0), ("dbeta", db, db64, s1, db0)):
        b = (U + S64) * (np.abs(s[0]) + np.abs(s[1])) + U * (np.abs(init + s[0]) + np.abs(ref))
        ratios[name] = float((np.abs(out.t.cpu().double().numpy() - ref) / (b * slack)).max())
    assert dg.sentinels_intact() and db.sentinels_intact() and cf.sentinels_intact()
    with capsys.disabled():
        print("\nfloat-valued finalize, largest error / bound:", {k: round(v, 3) for k, v in ratios.items()})
    for name, r in ratios.items():
        assert r <= 1.0, (name, r)


# ---- the one-launch forms ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.FUSED_CASES, ids=[c[0] for c in R.FUSED_CASES])
def test_fused_forms_on_hand_made_slabs(ops, L, vg_switch, case):
    """vg_bn_finalize_act_forward and vg_bn_backward_finalize_apply == the restatement == the separate kernels, bit for bit:
    outputs, published coefficients, running statistics, dgamma / dbeta."""
    vg_switch("VG_BN_FUSED_FWD", 1)
    name, rpg, groups, C, nparts, act, slope = case
    d, fw, bw = R.fused_inputs(case)
    lib, sp, rows, dtype = L.load(), L.stream_ptr(), rpg * groups, R.BF16
    assert ops.bn_launch_plan("fused", rows, C, dtype, groups, nparts=nparts)["fused"]
    X, DY = dev(d["x"], torch.bfloat16), dev(d["dy"], torch.bfloat16)
    S, gm, bt = dev(fw["slabs"]), dev(fw["gamma"]), dev(fw["beta"])
    co_ref, rm_ref, rv_ref = R.finalize(*R.slab_sums(fw["slabs"]), rpg, fw["gamma"], fw["beta"], fw["rmean"], fw["rvar"],
                                        fw["momentum"], fw["eps"])
    y_ref = R.forward(d["x"], co_ref[:, 2], co_ref[:, 3], act, slope, dtype, groups)
    rm, rv = _running(fw)
    y, co = Out((rows, C), torch.bfloat16), Out((groups, 4, C))
    check(L, lib.vg_bn_finalize_act_forward(X.data_ptr(), y.ptr(), S.data_ptr(), nparts, groups, C, rows, gm.data_ptr(),
                                            bt.data_ptr(), rm.ptr(), rv.ptr(), fw["momentum"], fw["eps"], co.ptr(), act, slope,
                                            dtype, sp), "vg_bn_finalize_act_forward")
    assert_bits(y, y_ref, "fused forward y"), assert_bits(co, co_ref, "fused forward coefficients")
    assert_bits(rm, rm_ref, "fused running mean"), assert_bits(rv, rv_ref, "fused running var")
    rm2, rv2 = _running(fw)
    y2, co2 = Out((rows, C), torch.bfloat16), Out((groups, 4, C))
    check(L, lib.vg_bn_finalize_grouped(S.data_ptr(), nparts, groups, C, rpg, gm.data_ptr(), bt.data_ptr(), rm2.ptr(), rv2.ptr(),
                                        fw["momentum"], fw["eps"], co2.ptr(), sp), "vg_bn_finalize_grouped")
    check(L, lib.vg_bn_act_forward(X.data_ptr(), y2.ptr(), co2.ptr(2 * C), co2.ptr(3 * C), rows, C, act, slope, groups, 4 * C,
                                   dtype, sp), "vg_bn_act_forward")
    for a, b, what in ((y, y2, "y"), (co, co2, "coefficients"), (rm, rm2, "running mean"), (rv, rv2, "running var")):
        assert torch.equal(a.t.view(BITS[a.t.dtype]), b.t.view(BITS[b.t.dtype])), "fused != separate: " + what
    # backward twin: the coefficients handed in are the stream table's, b and c come from the slabs
    CO, P, gmb = dev(d["coeffs"]), dev(bw["slabs"]), dev(bw["gamma"])
    dg_ref, db_ref, cf_ref = R.bwd_finalize(*R.slab_sums(bw["slabs"]), rpg, bw["gamma"], bw["invstd"], bw["dgamma"], bw["dbeta"], 1)
    dx_ref = R.apply(d["x"], d["dy"], d["coeffs"], cf_ref, act, slope, dtype, groups)
    dg, db = _grads(bw)
    dx = Out((rows, C), torch.bfloat16)
    check(L, lib.vg_bn_backward_finalize_apply(X.data_ptr(), DY.data_ptr(), dx.ptr(), P.data_ptr(), nparts, groups, C, rows,
                                               gmb.data_ptr(), CO.data_ptr(), dg.ptr(), db.ptr(), 1, act, slope, dtype, sp),
          "vg_bn_backward_finalize_apply")
    assert_bits(dx, dx_ref, "fused backward dx")
    assert_bits(dg, dg_ref, "fused backward dgamma"), assert_bits(db, db_ref, "fused backward dbeta")
    dg2, db2 = _grads(bw)
    dx2, cf2 = Out((rows, C), torch.bfloat16), Out((groups, 3, C))
    check(L, lib.vg_bn_backward_finalize_grouped(P.data_ptr(), nparts, groups, C, rpg, gmb.data_ptr(), CO.data_ptr(), dg2.ptr(),
                                                 db2.ptr(), 1, cf2.ptr(), sp), "vg_bn_backward_finalize_grouped")
    check(L, lib.vg_bn_act_backward_apply(X.data_ptr(), DY.data_ptr(), dx2.ptr(), CO[0, 2].data_ptr(), CO[0, 3].data_ptr(),
                                          CO[0, 0].data_ptr(), CO[0, 1].data_ptr(), cf2.ptr(), rows, C, act, slope, groups, 4 * C,
                                          3 * C, dtype, sp), "vg_bn_act_backward_apply")
    assert_bits(cf2, cf_ref, "separate backward coef")
    for a, b, what in ((dx, dx2, "dx"), (dg, dg2, "dgamma"), (db, db2, "dbeta")):
        assert torch.equal(a.t.view(BITS[a.t.dtype]), b.t.view(BITS[b.t.dtype])), "fused != separate: " + what
    # a refused shape is an error, not a fallback
    assert lib.vg_bn_finalize_act_forward(X.data_ptr(), y.ptr(), S.data_ptr(), 201, groups, C, rows, gm.data_ptr(), bt.data_ptr(),
                                          None, None, 0.5, 0.0, co.ptr(), act, slope, dtype, sp) == L.VG_ENOSUP


# ---- the chain through ops.py ---------------------------------------------------------------------------------------------
def _chain(ops, X, DY, gm, bt, rm, rv, rpg, groups, C, act, slope, dtype, mom, eps):
    rows = rpg * groups
    slabs = []
    for k in range(groups):
        st, n = ops.channel_stats(X[k * rpg:(k + 1) * rpg], rpg, C, dtype)
        slabs.append(st[:n * 2 * C].clone())
    stats = torch.cat(slabs)
    r = ops.bn_finalize_act_forward(X, stats, n * groups, C, rows, gm, bt, rm, rv, mom, eps, act, slope, dtype, groups)
    if r is None:
        co = ops.bn_finalize(stats, n * groups, C, rows, gm, bt, rm, rv, mom, eps, X.device, groups=groups)
        y = ops.bn_act_forward(X, co, rows, C, act, slope, dtype)
    else:
        co, y = r
    dg, db = torch.zeros(C, device=X.device), torch.zeros(C, device=X.device)
    dx = ops.bn_act_backward(X, DY, co, rows, C, rows, gm, act, slope, dg, db, False, dtype)
    return dict(coeffs=co, y=y, dx=dx, dgamma=dg, dbeta=db, fused=r is not None)


@pytest.mark.parametrize("fused", [0, 1], ids=["separate", "fused"])
@pytest.mark.parametrize("dtype", [R.F32, R.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", R.CHAIN_CASES, ids=[c[0] for c in R.CHAIN_CASES])
def test_chain_on_two_point_data(ops, vg_switch, case, dtype, fused):
    """stats -> finalize -> forward -> reduce -> bwd-finalize -> apply through ops.py on data whose statistics are exact, with
    the one-launch forms on and off; one case is replayed once from a hipGraph and must equal its eager run."""
    vg_switch("VG_BN_FUSED_FWD", fused)
    vg_switch("VG_BN_ONEPASS", 0)
    name, rpg, groups, C, act, slope = case
    d = R.chain_inputs(case)
    want = R.chain_ref(d, rpg, groups, C, act, slope, dtype)
    X, DY, gm, bt = dev(d["x"], TD[dtype]), dev(d["dy"], TD[dtype]), dev(d["gamma"]), dev(d["beta"])
    rm, rv = dev(d["rmean"]), dev(d["rvar"])
    got = _chain(ops, X, DY, gm, bt, rm, rv, rpg, groups, C, act, slope, dtype, d["momentum"], d["eps"])
    took = ops.bn_launch_plan("fused", rpg * groups, C, dtype, groups,
                              nparts=ops.bn_launch_plan("reduce", rpg * groups, C, dtype, groups)["blocks_per_group"])["fused"]
    assert got["fused"] == took == bool(fused and dtype == R.BF16 and C % 64 == 0)
    for k in ("coeffs", "y", "dx", "dgamma", "dbeta"):
        assert_bits(got[k], want[k], f"chain {k}")
    assert_bits(rm, want["rmean"], "chain running mean"), assert_bits(rv, want["rvar"], "chain running var")
    if name == "ch128_g2" and dtype == R.BF16 and fused:
        C_ = importlib.import_module(PKG + ".capture")
        rm_s, rv_s = dev(d["rmean"]), dev(d["rvar"])
        step = lambda x, dy, a, b: _chain(ops, x, dy, gm, bt, a, b, rpg, groups, C, act, slope, dtype, d["momentum"], d["eps"])
        cap = C_.capture(step, (X, DY, rm_s, rv_s), C_.HostMirrors([], []), torch.device(DEV, torch.cuda.current_device()))
        assert torch.equal(rm_s, dev(d["rmean"])), "a capture executes nothing"
        C_.replay(cap)
        torch.cuda.synchronize()
        for k in ("coeffs", "y", "dx", "dgamma", "dbeta"):
            assert torch.equal(cap.out[k].view(BITS[cap.out[k].dtype]), got[k].view(BITS[got[k].dtype])), f"replay != eager: {k}"
        assert torch.equal(rm_s, rm) and torch.equal(rv_s, rv), "replay != eager: running statistics"
