"""GPU: vg_gather_gemm on integer operands against torch's f64 convolutions (tests/_gg_ref.py), bit for bit.

Every real channel of the input and of the weights holds +-1, +-2 or +-3 (+-1 for fp8 operands and for long K), the bias small
integers, the slopes powers of two: every product, partial sum and statistics sum is an integer (or a multiple of 1/4) below
2^24, so f32 adds them exactly in ANY order.  Whatever tile, staging, patch kernel, split count or reduce a case takes, it has
to produce the reference's bits -- output (padding channels included) and statistics slabs; a mismatch is a wrong, missing or
doubled term or a wrong rounding, never noise, and the difference names it.  Before the launch the library's plan
(vg_gather_gemm_plan, the record the launcher launches from) must be the kernel the row is in the table for; after it the
launch count must be 1, or 2 with a slab reduce.  The table's coverage of the launcher is asserted in tests/test_gg_cpu.py."""
import functools
import importlib

import pytest
import torch

import _gg_ref as R

pytestmark = pytest.mark.gpu

G = R.G
DEV = "cuda"
SWITCH_NAMES = sorted({n for c in R.ALL_CASES for n in c.switches})


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return importlib.import_module(R.PKG + ".ops")


@functools.lru_cache(maxsize=None)
def _problem(case):
    """Operands and references of one row: computed once, never modified."""
    o = R.operands(case)
    yf = R.preact_ref(case, o)
    return o, yf, R.output_ref(case, o, yf)


def _first(got, ref, names):
    bad = (got != ref) | (got.isnan() != ref.isnan())
    idx = tuple(int(v) for v in bad.nonzero()[0])
    a, b = float(got[idx]), float(ref[idx])
    return (f"{int(bad.sum())} of {ref.numel()} elements differ; first at ({', '.join(f'{n} {i}' for n, i in zip(names, idx))}): "
            f"kernel {a}, reference {b}, difference {a - b}")


def _check(ops, vg_switch, monkeypatch, case):
    for n in SWITCH_NAMES:
        monkeypatch.delenv(n, raising=False)
    for n, v in case.switches.items():
        vg_switch(n, v)
    g, pk = case.specs()
    o, yf, Yref = _problem(case)
    assert (R.written_mask(g) == 1).all()               # (tests/test_gg_cpu.py: no builder leaves an output pixel unwritten)
    plan = ops.gather_gemm_plan(g, case.dtype, bias=case.has("b"), want_stats=case.has("s"), act=case.act, mask=case.mask)
    assert R.label(plan) == case.label, plan
    assert R.exactness(case, o, yf, plan["bm"]) == []

    st_dt = G.BF16 if case.dtype == G.FP8 else case.dtype
    X = R.x_nhwc(case, o["x"]).to(DEV)
    Wp = ops.pack_weights(pk, o["w"].float().flatten().to(DEV), st_dt)
    if case.dtype == G.FP8:
        X, Wp = ops.cast_fp8(X), ops.cast_fp8(Wp, 6)
    bias = None if o["bias"] is None else o["bias"].float().to(DEV)
    mask = None if case.mask is None else (o["mask"].to(Yref.dtype).to(DEV),) + case.mask
    out = torch.full(Yref.shape, float("nan"), dtype=Yref.dtype, device=DEV)
    if case.has("s"):                                   # the slab buffer gather_gemm hands out: stale rows must not pass for written ones
        ops.WS.get("stats", plan["nparts"] * 2 * g.N * 4, X.device).fill_(float("nan"))
    n0 = ops.launch_count()
    Y, stats, nparts = ops.gather_gemm(g, X, Wp, case.dtype, bias=bias, want_stats=case.has("s"), out=out, act=case.act,
                                       mask=mask)
    launches = ops.launch_count() - n0
    torch.cuda.synchronize()
    assert launches == (2 if plan["ksplit"] > 1 else 1), (launches, plan)
    got = Y.view(Yref.shape).cpu()
    assert torch.equal(got, Yref), "output: " + _first(got.double(), Yref.double(), ("b", "oy", "ox", "n"))
    if case.has("s"):
        assert nparts == plan["nparts"]
        ref = R.stats_ref(g, yf, plan["bm"]).float()
        got = stats[: nparts * 2 * g.N].view(nparts, 2, g.N).cpu()
        assert torch.equal(got, ref), "statistics: " + _first(got.double(), ref.double(), ("slab", "which", "n"))


@pytest.mark.parametrize("case", R.CASES, ids=[c.id for c in R.CASES])
def test_gather_gemm_of_integer_operands_is_exact(ops, vg_switch, monkeypatch, case):
    _check(ops, vg_switch, monkeypatch, case)


@pytest.mark.parametrize("case", R.SWITCH_CASES, ids=[c.id for c in R.SWITCH_CASES])
def test_workgroup_order_gives_the_same_bits(ops, vg_switch, monkeypatch, case):
    """VG_GG_NMAJOR forced on (=2) and off (=0), where the n-tile count is a multiple of 8 and where it is not: each equals
    the reference, hence the other."""
    _check(ops, vg_switch, monkeypatch, case)
