"""GPU: vg_wgrad on integer operands against the f64 restatement of tests/_wgrad_ref.py, bit for bit.

Every real channel holds +-1, +-2 or +-3: the products are integers of magnitude <= 9 and every partial sum stays below 2^24,
so f32 adds them exactly in ANY order.  Whatever main kernel, split count, slab order or reduce kernel a case takes, it has
to produce the reference's bits; a mismatch is a wrong, missing or doubled term, never rounding, and the difference names
it (one product = one pixel row).  The case table (with the branch every row reaches) is in _wgrad_ref.py; before each
launch the launcher's own plan record has to name the kernels the row is there for, and each call has to issue exactly the
two launches of that plan.  The table's coverage of the launcher is asserted in tests/test_wgrad_cpu.py."""
import functools
import importlib
import json
import os

import pytest
import torch

import _wgrad_ref as R

pytestmark = pytest.mark.gpu

G = R.G
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module(R.PKG + ".ops")


@functools.lru_cache(maxsize=None)
def _problem(case, dtype):
    """Operands, the integer tensor to accumulate onto and the f64 reference of one (case, dtype): computed once, shared by
    both tests, never modified."""
    wg = case.spec(dtype)
    P, Q = R.int_operands(wg, dtype, 1)
    ref = R.wgrad_ref(wg, P, Q)
    assert float(ref.abs().max()) * 2 < 2 ** 24
    return wg, P, Q, R.int_dw(wg, 2), ref.float()


def _first_mismatch(wg, got, ref):
    i = int((got != ref).nonzero()[0])
    np_, rest = divmod(i, wg.s_np)
    cq, tap = divmod(rest, wg.s_cq)
    bad = int((got != ref).sum())
    return f"{bad} of {ref.numel()} elements differ; first at (np {np_}, cq {cq}, tap {tap}): kernel {float(got[i])}, " \
           f"reference {float(ref[i])}, difference {float(got[i]) - float(ref[i])}"


def _check(ops, case, dtype, kernels):
    wg, P, Q, d0, ref = _problem(case, dtype)
    assert R.label(ops.wgrad_plan(wg, dtype)) == kernels
    Pd, Qd = P.to(DEV), Q.to(DEV)
    dW = torch.full((ref.numel(),), float("nan"), device=DEV)
    n0 = ops.launch_count()
    ops.wgrad(wg, Pd, Qd, dW, False, dtype)
    assert ops.launch_count() - n0 == 2
    got = dW.cpu()
    assert torch.equal(got, ref), _first_mismatch(wg, got, ref)
    dW = d0.to(DEV)
    n0 = ops.launch_count()
    ops.wgrad(wg, Pd, Qd, dW, True, dtype)
    assert ops.launch_count() - n0 == 2
    got = dW.cpu()
    assert torch.equal(got, d0 + ref), "accumulate: " + _first_mismatch(wg, got, d0 + ref)


@pytest.mark.parametrize("case,dtype", R.CASE_PARAMS, ids=R.CASE_IDS)
def test_weight_gradient_of_integer_operands_is_exact(ops, vg_switch, case, dtype):
    if case.target:
        vg_switch("VG_WG_TARGET", case.target)
    _check(ops, case, dtype, case.kernels(dtype))


@functools.lru_cache(maxsize=None)
def _switched_kernels():
    """id of a SWITCH_PARAMS row -> (main, reduce) it reached at the parent commit (tools/gen_golden_wg_plan.py)."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wg_plan_parent.json")) as f:
        return {k: (v["main"], v["reduce"]) for k, v in json.load(f)["switches"].items()}


@pytest.mark.parametrize("case,dtype,switch,value", R.SWITCH_PARAMS, ids=R.SWITCH_IDS)
def test_every_build_of_the_weight_gradient_gives_the_same_bits(ops, vg_switch, case, dtype, switch, value):
    """The non-default main kernels (VG_WG_SPEC, VG_WG_DMA), the generic reduce in place of the streaming one
    (VG_WG_REDUCE_T), other split counts (VG_WG_TARGET) and the forced XCD order: each equals the reference exactly, hence
    every other variant."""
    vg_switch(switch, value)
    _check(ops, case, dtype, _switched_kernels()[f"{case.id}-{R.DT_NAME[dtype]}-{switch}={value}"])
