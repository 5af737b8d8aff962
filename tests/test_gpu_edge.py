"""GPU: vg_tnconv and vg_edge_wgrad on integer operands against the f64 restatements of tests/_edge_ref.py, bit for bit.

Every operand element is +-1, +-2 or +-3: products are integers of magnitude <= 9 and every partial sum stays far below 2^24,
so f32 adds them exactly in ANY order.  Whatever tiling, halo window, column block or workgroup walk a row takes, it has to
produce the reference's bits; a mismatch is a wrong, missing or doubled term, never rounding, and the report names its pixel.
The case tables (with the facet of the planners every row is there for) are in _edge_ref.py; before each launch the launcher's
own plan record has to show the tiling the row is listed with, and each call has to issue exactly the launches of that plan
(1 for vg_tnconv, 2 for vg_edge_wgrad).  The tables' coverage of the launchers is asserted in tests/test_edge_cpu.py; the
real-valued epilogue (tanh) stays with the tolerance tests of tests/test_gpu_kernels.py."""
import functools
import importlib

import pytest
import torch

import _edge_ref as E
import _wgrad_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module(R.PKG + ".ops")


# ---- vg_tnconv -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tn_problem(case):
    """Specs, operands, integer noise, its scale and the f64 reference [B][N][OH][OW] of one row: computed once, shared by the
    tests, never modified."""
    tn, pk = case.spec()
    X, W = E.tn_operands(tn, 1)
    ref = E.tnconv_ref(tn, X, W)
    assert 2 * float(ref.abs().max()) < 2 ** 24
    return tn, pk, X, W, E.tn_eps(tn, 2), E.tn_sigma(ref), ref


def _tn_mismatch(got, ref):
    """got, ref: [B][N][OH][OW] of one dtype."""
    bad = got != ref
    b, n, oy, ox = (int(i) for i in bad.nonzero()[0])
    g, r = float(got[b, n, oy, ox]), float(ref[b, n, oy, ox])
    return f"{int(bad.sum())} of {ref.numel()} elements differ; first at (b {b}, oy {oy}, ox {ox}, n {n}): kernel {g}, " \
           f"reference {r}, difference {g - r}"


def _nchw(y_nhwc, N):
    return y_nhwc[..., :N].permute(0, 3, 1, 2).contiguous()


def _tn_run(ops, case, tn, Xd, wp, **kw):
    """One launch into a NaN-filled NHWC buffer -> (Y NHWC on the host, Y_nchw on the host or None)."""
    out = torch.full((tn.B, tn.OH, tn.OW, tn.OC), NAN, dtype=torch.bfloat16, device=DEV)
    n0 = ops.launch_count()
    y, img = ops.tnconv(tn, Xd, wp, out_nhwc=out, **kw)
    assert ops.launch_count() - n0 == 1
    assert y.data_ptr() == out.data_ptr()
    y = y.cpu()
    assert not torch.isnan(y.float()).any(), f"{int(torch.isnan(y.float()).sum())} elements of Y were not written"
    assert (y[..., tn.N:] == 0).all(), "padding channels of Y are not zero"
    return y, None if img is None else img.cpu()


@pytest.mark.parametrize("case", E.TN_CASES, ids=E.TN_IDS)
def test_transposed_conv_of_integer_operands_is_exact(ops, case):
    tn, pk, X, W, eps, sigma, ref = _tn_problem(case)
    assert E.tn_plan_tuple(ops.tnconv_plan(tn)) == case.plan
    Xd, wp = X.to(DEV), ops.pack_weights(pk, W.to(DEV), R.G.BF16)
    # plain: Y_nchw is the f32 sum itself, Y its nearest-even bf16 rounding
    y, img = _tn_run(ops, case, tn, Xd, wp, want_nchw=True)
    assert torch.equal(img, ref.float()), "Y_nchw: " + _tn_mismatch(img, ref.float())
    want = ref.float().to(torch.bfloat16)
    assert torch.equal(_nchw(y, tn.N), want), "Y: " + _tn_mismatch(_nchw(y, tn.N), want)
    # injected noise: Y = bf16(v + sigma*eps) with every term exact, Y_nchw stays v
    assert sigma > E.bf16_spacing(float(ref.abs().max()))
    y, img = _tn_run(ops, case, tn, Xd, wp, want_nchw=True, noise=eps.to(DEV), sigma=sigma)
    assert torch.equal(img, ref.float()), "Y_nchw beside the noisy Y: " + _tn_mismatch(img, ref.float())
    want = (ref + sigma * eps.double()).float().to(torch.bfloat16)
    assert torch.equal(_nchw(y, tn.N), want), "noisy Y: " + _tn_mismatch(_nchw(y, tn.N), want)
    # the NHWC output alone (no Y_nchw pointer)
    y, img = _tn_run(ops, case, tn, Xd, wp)
    want = ref.float().to(torch.bfloat16)
    assert img is None and torch.equal(_nchw(y, tn.N), want), "Y alone: " + _tn_mismatch(_nchw(y, tn.N), want)


@pytest.mark.parametrize("case", E.TN_RNG_CASES, ids=E.TN_RNG_IDS)
def test_transposed_conv_noise_drawn_in_kernel_equals_the_materialised_draw(ops, case):
    """The rows whose tiling changes with in-kernel noise (column step 4, lane quads share a Philox block) and the rows whose
    output width is no multiple of 4 (no quads: one draw per element): the same bits as the draw materialised by vg_randn and
    injected -- under the OTHER plan -- and Y_nchw is still the exact sum."""
    tn, pk, X, W, _, sigma, ref = _tn_problem(case)
    plan = ops.tnconv_plan(tn, rng=True)
    assert E.tn_plan_tuple(plan) == case.rng_plan and plan["quad_noise"] == (tn.OW % 4 == 0)
    Xd, wp = X.to(DEV), ops.pack_weights(pk, W.to(DEV), R.G.BF16)
    ns = ops.NoiseStream(DEV, 77)
    ns.advance()
    eps = ns.randn((tn.B, tn.N, tn.OH, tn.OW), 2)
    ym, _ = _tn_run(ops, case, tn, Xd, wp, want_nchw=True, noise=eps, sigma=sigma)
    yr, img = _tn_run(ops, case, tn, Xd, wp, want_nchw=True, noise=ns.draw(2), sigma=sigma)
    assert torch.equal(img, ref.float()), "Y_nchw: " + _tn_mismatch(img, ref.float())
    assert not torch.equal(_nchw(ym, tn.N), ref.float().to(torch.bfloat16)), "the noise does not show in Y"
    assert torch.equal(yr, ym), "in-kernel draw against the injected one: " + _tn_mismatch(_nchw(yr, tn.N).float(), _nchw(ym, tn.N).float())


# ---- vg_edge_wgrad -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ew_problem(case):
    ew = case.spec()
    wide, narrow = E.ew_operands(ew, 1)
    ref = E.edge_wgrad_ref(ew, wide, narrow)
    assert 2 * float(ref.abs().max()) < 2 ** 24
    return ew, wide, narrow, E.ew_int_dw(ew, 2), ref.float()


def _ew_mismatch(ew, got, ref):
    bad = got != ref
    i = int(bad.nonzero()[0])
    c, rest = divmod(i, ew.s_c)
    n, tap = divmod(rest, ew.s_n)
    return f"{int(bad.sum())} of {ref.numel()} elements differ; first at (c {c}, n {n}, kh {tap // ew.K}, kw {tap % ew.K}): " \
           f"kernel {float(got[i])}, reference {float(ref[i])}, difference {float(got[i]) - float(ref[i])}"


@pytest.mark.parametrize("case", E.EW_CASES, ids=E.EW_IDS)
def test_edge_weight_gradient_of_integer_operands_is_exact(ops, case):
    ew, wide, narrow, d0, ref = _ew_problem(case)
    plan = ops.edge_wgrad_plan(ew)
    assert E.ew_plan_tuple(plan) == case.plan
    wd, nd = wide.to(DEV), narrow.to(DEV)
    for accumulate, start, want in ((False, torch.full_like(ref, NAN), ref), (True, d0, d0 + ref)):
        # the partials of another launch must not be read: the shared workspace holds NaN wherever this one does not write
        ops.WS.get("wgrad", plan["ws_bytes"], wd.device).fill_(NAN)              # (the buffer ops.edge_wgrad fetches)
        dW = start.to(DEV)
        n0 = ops.launch_count()
        ops.edge_wgrad(ew, wd, nd, dW, accumulate)
        assert ops.launch_count() - n0 == 2
        got = dW.cpu()
        assert torch.equal(got, want), ("accumulate: " if accumulate else "") + _ew_mismatch(ew, got, want)
